// Micro-benchmark: how the carry of one product-scanning column should reach the next column (csrc/h2v_field.hpp, fp_mont28 and
// fp_montsqr28).  The source keeps one rolling accumulator (acc >>= 28, then acc += a[i] * b[k - i]), but the optimiser
// reassociates each column's sum so that the products come first and the carry is added last with a separate 64-bit addition
// (v_lshl_add_u64 with shift 0): 27 per product.  The forms below keep the carry as the addend of the column's first
// v_mad_u64_u32; they differ in what the compiler's hazard recogniser puts behind them (it assumes that an inline-asm statement
// forwards its destination like an SDWA write, and separates it from a VALU reader of its output by one s_nop).
//   a  plain     today's source
//   b  asm-mad   every multiply-add a one-instruction asm statement
//   c  barrier   plain multiply-add, then an empty asm statement that makes the partial sum opaque
//   d  asm-run   up to 8 multiply-adds of a column in one asm statement (1 + 2 x 8 + 2 = 19 of the 30 operands a statement may have)
//   e  copy      plain multiply-add, then llvm.amdgcn.softwqm on the partial sum (all but the column's last): opaque to the IR
//                passes, and in a kernel without whole-quad mode (every compute kernel) the backend lowers it to a COPY that the
//                register coalescer removes: no instruction, no asm statement, no s_nop
// Method as tools/ubench/dfma_mont.hip: a chain of dependent products per lane, 1 / 2 / 4 waves per SIMD, 5 launches of >= 5 ms,
// cycles per reduced product per SIMD (s_memtime, median over the waves of a launch; min / median / max of the five launches), and
// every form checked bit for bit against a host big-integer a b R^-1 mod p on the same edge and random operands.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench/mont_carry.hip -o /tmp/mont_carry && /tmp/mont_carry
// (tools/scripts/gpu_ubench.sh also counts the instructions of each form's kernel from the compiled code.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

typedef unsigned __int128 u128;
static const uint64_t P64[6] = {0xb9feffffffffaaabull, 0x1eabfffeb153ffffull, 0x6730d2a0f6b0f624ull, 0x64774b84f38512bfull, 0x4b1ba7b6434bacd7ull, 0x1a0111ea397fe69aull};
static const uint64_t RINV28_64[6] = {0xd03433825937d5f3ull, 0x5bab6111a3ad18faull, 0x89b2c24e13432f44ull, 0x29e226de2c8bd445ull, 0x58dea736114b9b5aull, 0x1055a9f965d8eb2dull};  // 2^-392 mod p
static constexpr uint32_t P28[14] = {0xfffaaab, 0xfefffff, 0x3ffffb9, 0xfffeb15, 0x6241eab, 0xa0f6b0f, 0xf6730d2, 0xf38512b, 0x4774b84, 0x4bacd76, 0xba7b643, 0xe69a4b1, 0x1ea397f, 0x1a011};
#define N0_28 0xffcfffdu
#define M28 0xfffffffu
#define DI __device__ __forceinline__

enum { F_PLAIN = 0, F_ASM_MAD = 1, F_BARRIER = 2, F_ASM_RUN = 3, F_COPY = 4, N_FORMS = 5 };
static const char *FORM_NAME[N_FORMS] = {"a-plain", "b-asm-mad", "c-barrier", "d-asm-run", "e-copy"};

extern "C" __device__ uint64_t mc_soft_copy(uint64_t) __asm("llvm.amdgcn.softwqm.i64");

// ---- one multiply-add into the column, per form.  P: the second factor is a modulus limb (a compile-time constant; an asm
// statement needs it in an SGPR, since v_mad_u64_u32 takes no literal and a "v" input would cost a v_mov per limb)
template <int F, bool P> DI void mac(uint64_t &acc, uint32_t x, uint32_t y) {
    if (F == F_ASM_MAD) {
        uint64_t co;
        if (P) asm("v_mad_u64_u32 %0, %1, %2, %3, %0" : "+v"(acc), "=&s"(co) : "v"(x), "s"(y));
        else asm("v_mad_u64_u32 %0, %1, %2, %3, %0" : "+v"(acc), "=&s"(co) : "v"(x), "v"(y));
        return;
    }
    acc += (uint64_t)x * y;
    if (F == F_BARRIER) asm("" : "+v"(acc));
    if (F == F_COPY) acc = mc_soft_copy(acc);
}
// the LAST term of a column.  Form e leaves it plain, as the library does: two addends cannot be reassociated, and the column's value
// is then the multiply-add's own result instead of a copy of it (which cost a v_mov per column of the upper half)
template <int F, bool P> DI void mac_end(uint64_t &acc, uint32_t x, uint32_t y) {
    if (F == F_COPY) acc += (uint64_t)x * y;
    else mac<F, P>(acc, x, y);
}
// ---- form d: N multiply-adds x[i] * y[-i] in statements of 8, 4, 2 and 1 (x walks up, y down)
#define MC_MAD "v_mad_u64_u32 %0, %1, "
template <int N, bool P> DI void mac_run(uint64_t &acc, const uint32_t *x, const uint32_t *y) {
    uint64_t co;
    if constexpr (N >= 8) {
        if (P) asm(MC_MAD "%2, %10, %0\n\t" MC_MAD "%3, %11, %0\n\t" MC_MAD "%4, %12, %0\n\t" MC_MAD "%5, %13, %0\n\t"
                   MC_MAD "%6, %14, %0\n\t" MC_MAD "%7, %15, %0\n\t" MC_MAD "%8, %16, %0\n\t" MC_MAD "%9, %17, %0"
                   : "+v"(acc), "=&s"(co) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]),
                     "s"(y[0]), "s"(y[-1]), "s"(y[-2]), "s"(y[-3]), "s"(y[-4]), "s"(y[-5]), "s"(y[-6]), "s"(y[-7]));
        else asm(MC_MAD "%2, %10, %0\n\t" MC_MAD "%3, %11, %0\n\t" MC_MAD "%4, %12, %0\n\t" MC_MAD "%5, %13, %0\n\t"
                 MC_MAD "%6, %14, %0\n\t" MC_MAD "%7, %15, %0\n\t" MC_MAD "%8, %16, %0\n\t" MC_MAD "%9, %17, %0"
                 : "+v"(acc), "=&s"(co) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]),
                   "v"(y[0]), "v"(y[-1]), "v"(y[-2]), "v"(y[-3]), "v"(y[-4]), "v"(y[-5]), "v"(y[-6]), "v"(y[-7]));
        mac_run<N - 8, P>(acc, x + 8, y - 8);
    } else if constexpr (N >= 4) {
        if (P) asm(MC_MAD "%2, %6, %0\n\t" MC_MAD "%3, %7, %0\n\t" MC_MAD "%4, %8, %0\n\t" MC_MAD "%5, %9, %0"
                   : "+v"(acc), "=&s"(co) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "s"(y[0]), "s"(y[-1]), "s"(y[-2]), "s"(y[-3]));
        else asm(MC_MAD "%2, %6, %0\n\t" MC_MAD "%3, %7, %0\n\t" MC_MAD "%4, %8, %0\n\t" MC_MAD "%5, %9, %0"
                 : "+v"(acc), "=&s"(co) : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(y[0]), "v"(y[-1]), "v"(y[-2]), "v"(y[-3]));
        mac_run<N - 4, P>(acc, x + 4, y - 4);
    } else if constexpr (N >= 2) {
        if (P) asm(MC_MAD "%2, %4, %0\n\t" MC_MAD "%3, %5, %0" : "+v"(acc), "=&s"(co) : "v"(x[0]), "v"(x[1]), "s"(y[0]), "s"(y[-1]));
        else asm(MC_MAD "%2, %4, %0\n\t" MC_MAD "%3, %5, %0" : "+v"(acc), "=&s"(co) : "v"(x[0]), "v"(x[1]), "v"(y[0]), "v"(y[-1]));
        mac_run<N - 2, P>(acc, x + 2, y - 2);
    } else if constexpr (N == 1) {
        mac<F_ASM_MAD, P>(acc, x[0], y[0]);
    }
}

// t = a b / 2^392 mod p (below 2p): the multiplier of csrc/h2v_field.hpp, fp_mont28, with the multiply-add of form F
template <int F> DI void mont(uint32_t (&t)[14], const uint32_t (&a)[14], const uint32_t (&b)[14]) {
    uint32_t m[14];
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 14; k++) {
#pragma unroll
        for (int i = 0; i <= k; i++) mac<F, false>(acc, a[i], b[k - i]);
#pragma unroll
        for (int i = 0; i < k; i++) mac<F, true>(acc, m[i], P28[k - i]);
        m[k] = ((uint32_t)acc * N0_28) & M28;
        mac_end<F, true>(acc, m[k], P28[0]);
        acc >>= 28;
    }
#pragma unroll
    for (int k = 14; k < 27; k++) {
#pragma unroll
        for (int i = k - 13; i < 14; i++) mac<F, false>(acc, a[i], b[k - i]);
#pragma unroll
        for (int i = k - 13; i < 13; i++) mac<F, true>(acc, m[i], P28[k - i]);
        mac_end<F, true>(acc, m[13], P28[k - 13]);
        t[k - 14] = (uint32_t)acc & M28;
        acc >>= 28;
    }
    t[13] = (uint32_t)acc;
}
template <int K> DI void mont_run_low(uint64_t &acc, uint32_t (&m)[14], const uint32_t (&a)[14], const uint32_t (&b)[14]) {
    if constexpr (K < 14) {
        mac_run<K + 1, false>(acc, &a[0], &b[K]);
        mac_run<K, true>(acc, &m[0], &P28[K]);
        m[K] = ((uint32_t)acc * N0_28) & M28;
        mac<F_ASM_MAD, true>(acc, m[K], P28[0]);
        acc >>= 28;
        mont_run_low<K + 1>(acc, m, a, b);
    }
}
template <int K> DI void mont_run_high(uint64_t &acc, uint32_t (&t)[14], const uint32_t (&m)[14], const uint32_t (&a)[14], const uint32_t (&b)[14]) {
    if constexpr (K < 27) {
        mac_run<27 - K, false>(acc, &a[K - 13], &b[13]);
        mac_run<27 - K, true>(acc, &m[K - 13], &P28[13]);
        t[K - 14] = (uint32_t)acc & M28;
        acc >>= 28;
        mont_run_high<K + 1>(acc, t, m, a, b);
    }
}
template <> DI void mont<F_ASM_RUN>(uint32_t (&t)[14], const uint32_t (&a)[14], const uint32_t (&b)[14]) {
    uint32_t m[14];
    uint64_t acc = 0;
    mont_run_low<0>(acc, m, a, b);
    mont_run_high<14>(acc, t, m, a, b);
    t[13] = (uint32_t)acc;
}
// t = a^2 / 2^392 mod p: fp_montsqr28 (off-diagonal products once, against the doubled operand).  Form d is not written out
// for the squaring: its columns are the same runs, half as long.
template <int F> DI void montsqr(uint32_t (&t)[14], const uint32_t (&a)[14]) {
    uint32_t m[14], d[14];
#pragma unroll
    for (int i = 0; i < 14; i++) d[i] = a[i] << 1;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 14; k++) {
#pragma unroll
        for (int i = 0; 2 * i < k; i++) mac<F, false>(acc, d[i], a[k - i]);
        if ((k & 1) == 0) mac<F, false>(acc, a[k / 2], a[k / 2]);
#pragma unroll
        for (int i = 0; i < k; i++) mac<F, true>(acc, m[i], P28[k - i]);
        m[k] = ((uint32_t)acc * N0_28) & M28;
        mac_end<F, true>(acc, m[k], P28[0]);
        acc >>= 28;
    }
#pragma unroll
    for (int k = 14; k < 27; k++) {
#pragma unroll
        for (int i = k - 13; 2 * i < k; i++) mac<F, false>(acc, d[i], a[k - i]);
        if ((k & 1) == 0) mac<F, false>(acc, a[k / 2], a[k / 2]);
#pragma unroll
        for (int i = k - 13; i < 13; i++) mac<F, true>(acc, m[i], P28[k - i]);
        mac_end<F, true>(acc, m[13], P28[k - 13]);
        t[k - 14] = (uint32_t)acc & M28;
        acc >>= 28;
    }
    t[13] = (uint32_t)acc;
}

// iters = 1: one product per lane (parity); otherwise a dependent chain x <- x y (SQ: x <- x^2) of `iters` products
template <int F, bool SQ, int MAXT> __global__ void __launch_bounds__(MAXT) k_chain(const uint32_t *in, uint32_t *out, uint64_t *stamps, uint32_t n, uint32_t iters) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, idx = gid < n ? gid : gid % n;
    uint32_t x[14], y[14];
#pragma unroll
    for (int i = 0; i < 14; i++) { x[i] = in[(size_t)idx * 28 + i]; y[i] = in[(size_t)idx * 28 + 14 + i]; }
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
#pragma unroll 1
    for (uint32_t it = 0; it < iters; it++) {
        uint32_t t[14];
        if (SQ) montsqr<F>(t, x); else mont<F>(t, x, y);
#pragma unroll
        for (int i = 0; i < 14; i++) x[i] = t[i];
    }
    const uint64_t t1 = __builtin_amdgcn_s_memtime();
    if (gid < n || iters > 1)
#pragma unroll
        for (int i = 0; i < 14; i++) out[(size_t)gid * 14 + i] = x[i];
    if (stamps && (threadIdx.x & 63) == 0) stamps[gid / 64] = t1 - t0;
}
template <int F, bool SQ> static void launch(int blocks, int threads, const uint32_t *in, uint32_t *out, uint64_t *st, uint32_t n, uint32_t iters) {
    if (threads == 256) k_chain<F, SQ, 256><<<blocks, threads>>>(in, out, st, n, iters);
    else if (threads == 512) k_chain<F, SQ, 512><<<blocks, threads>>>(in, out, st, n, iters);
    else k_chain<F, SQ, 1024><<<blocks, threads>>>(in, out, st, n, iters);
}
typedef void (*launch_fn)(int, int, const uint32_t *, uint32_t *, uint64_t *, uint32_t, uint32_t);
static const launch_fn MUL[N_FORMS] = {launch<F_PLAIN, false>, launch<F_ASM_MAD, false>, launch<F_BARRIER, false>, launch<F_ASM_RUN, false>, launch<F_COPY, false>};
static const launch_fn SQR[N_FORMS] = {launch<F_PLAIN, true>, launch<F_ASM_MAD, true>, launch<F_BARRIER, true>, nullptr, launch<F_COPY, true>};

// ---- host big integers (6 x 64 bits), slow and plain: the checker (as in dfma_mont.hip)
struct B384 { uint64_t w[6]; };
static int cmp(const B384 &a, const B384 &b) { for (int i = 5; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1; return 0; }
static B384 P() { B384 p; memcpy(p.w, P64, 48); return p; }
static void sub_in(B384 &a, const B384 &b) { u128 br = 0; for (int i = 0; i < 6; i++) { u128 d = (u128)a.w[i] - b.w[i] - br; a.w[i] = (uint64_t)d; br = (d >> 64) & 1; } }
static void add_mod(B384 &a, const B384 &b) {   // a, b < p
    u128 c = 0;
    for (int i = 0; i < 6; i++) { c += (u128)a.w[i] + b.w[i]; a.w[i] = (uint64_t)c; c >>= 64; }
    const B384 p = P();
    if (c || cmp(a, p) >= 0) sub_in(a, p);
}
static B384 mul_mod(const B384 &a, const B384 &b) {   // double-and-add over the bits of b
    B384 r = {};
    for (int bit = 383; bit >= 0; bit--) {
        add_mod(r, r);
        if ((b.w[bit / 64] >> (bit % 64)) & 1) add_mod(r, a);
    }
    return r;
}
static B384 reduce_mod(B384 a) { const B384 p = P(); while (cmp(a, p) >= 0) sub_in(a, p); return a; }
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static B384 rand_below_p() { B384 a; for (int i = 0; i < 6; i++) a.w[i] = rnd(); a.w[5] &= (1ull << 61) - 1; return reduce_mod(reduce_mod(a)); }
static void to_limbs28(const B384 &a, uint32_t *out) {
    for (int i = 0; i < 14; i++) {
        const int lo = 28 * i;
        u128 v = (u128)a.w[lo / 64];
        if (lo / 64 + 1 < 6) v |= (u128)a.w[lo / 64 + 1] << 64;
        out[i] = (uint32_t)(v >> (lo % 64)) & M28;
    }
}
static B384 from_limbs28(const uint32_t *l) {   // value below 2p
    B384 r = {};
    for (int i = 0; i < 14; i++) {
        const int lo = 28 * i;
        u128 v = (u128)l[i] << (lo % 64);
        u128 c = (u128)r.w[lo / 64] + (uint64_t)v;
        r.w[lo / 64] = (uint64_t)c;
        u128 carry = (c >> 64) + (v >> 64);
        for (int q = lo / 64 + 1; q < 6 && carry; q++) { c = (u128)r.w[q] + (uint64_t)carry; r.w[q] = (uint64_t)c; carry = c >> 64; }
    }
    return r;
}

struct Timing { double lo, med, hi; };
static Timing timed(const char *what, const char *name, int wps, launch_fn fn, const uint32_t *d_in, uint32_t *d_out, uint64_t *d_st, uint32_t n) {
    const int threads = wps >= 4 ? 1024 : 256 * wps, blocks = 256 * (wps >= 4 ? wps / 4 : 1);
    const size_t waves = (size_t)blocks * threads / 64;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    auto once = [&](uint32_t iters) { (void)hipEventRecord(e0); fn(blocks, threads, d_in, d_out, d_st, n, iters); (void)hipEventRecord(e1); (void)hipDeviceSynchronize(); float ms; (void)hipEventElapsedTime(&ms, e0, e1); return ms; };
    uint32_t iters = 256;
    float ms = once(iters);
    while (ms < 5.0f && iters < (1u << 20)) { iters = (uint32_t)(iters * (ms > 0.05f ? 6.0f / ms : 16.0f)) + 1; ms = once(iters); }
    std::vector<float> t;
    std::vector<double> cyc;
    for (int rep = 0; rep < 5; rep++) {
        t.push_back(once(iters));
        std::vector<uint64_t> h(waves);
        (void)hipMemcpy(h.data(), d_st, waves * 8, hipMemcpyDeviceToHost);
        std::sort(h.begin(), h.end());
        cyc.push_back((double)h[waves / 2] / ((double)iters * wps));
    }
    std::sort(t.begin(), t.end()); std::sort(cyc.begin(), cyc.end());
    printf("%-4s %-10s waves/SIMD=%d  %6u products per lane  median %.3f ms | cycles per reduced product per SIMD by s_memtime: %7.1f  (five launches %7.1f .. %7.1f) | %.0f by event time at 2.4 GHz\n",
           what, name, wps, iters, t[2], cyc[2], cyc[0], cyc[4], t[2] * 1e-3 * 2.4e9 / ((double)iters * wps));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return Timing{cyc[0], cyc[2], cyc[4]};
}

int main() {
    const uint32_t N = 10240;
    std::vector<B384> A(N), Bv(N);
    const B384 p = P();
    B384 pm1 = p; { B384 one = {{1, 0, 0, 0, 0, 0}}; sub_in(pm1, one); }
    std::vector<B384> edge;
    edge.push_back(B384{}); edge.push_back(B384{{1, 0, 0, 0, 0, 0}}); edge.push_back(pm1);
    for (int k = 0; k < 381; k += 13) { B384 e = {}; e.w[k / 64] = 1ull << (k % 64); edge.push_back(reduce_mod(e)); B384 f = e; sub_in(f, B384{{1, 0, 0, 0, 0, 0}}); if (k) edge.push_back(reduce_mod(f)); }
    { B384 e; for (int i = 0; i < 6; i++) e.w[i] = ~0ull; e.w[5] = (1ull << 60) - 1; edge.push_back(reduce_mod(e)); }   // all-ones limbs
    for (uint32_t i = 0; i < N; i++) {
        if (i < edge.size() * edge.size() && i < 4096) { A[i] = edge[i / edge.size()]; Bv[i] = edge[i % edge.size()]; }
        else { A[i] = rand_below_p(); Bv[i] = rand_below_p(); }
    }
    B384 rinv; memcpy(rinv.w, RINV28_64, 48);
    std::vector<uint32_t> in((size_t)N * 28);
    for (uint32_t i = 0; i < N; i++) { to_limbs28(A[i], &in[(size_t)i * 28]); to_limbs28(Bv[i], &in[(size_t)i * 28 + 14]); }
    const size_t max_threads = 256 * 1024;
    uint32_t *d_in, *d_out; uint64_t *d_st;
    if (hipMalloc(&d_in, in.size() * 4) != hipSuccess || hipMalloc(&d_out, max_threads * 14 * 4) != hipSuccess || hipMalloc(&d_st, max_threads / 64 * 8) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
    (void)hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice);
    // ---- parity: one product per lane, every form, against the host's a b R^-1 mod p (and a a R^-1 mod p)
    std::vector<B384> want_mul(N), want_sqr(N);
    for (uint32_t i = 0; i < N; i++) { want_mul[i] = mul_mod(mul_mod(A[i], Bv[i]), rinv); want_sqr[i] = mul_mod(mul_mod(A[i], A[i]), rinv); }
    std::vector<uint32_t> o((size_t)N * 14);
    uint32_t bad_total = 0;
    for (int sq = 0; sq < 2; sq++)
        for (int f = 0; f < N_FORMS; f++) {
            const launch_fn fn = sq ? SQR[f] : MUL[f];
            if (!fn) continue;
            (void)hipMemset(d_out, 0xff, (size_t)N * 14 * 4);
            fn((N + 255) / 256, 256, d_in, d_out, nullptr, N, 1);
            if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 1; }
            (void)hipMemcpy(o.data(), d_out, o.size() * 4, hipMemcpyDeviceToHost);
            uint32_t bad = 0;
            for (uint32_t i = 0; i < N; i++) {
                bool ok = cmp(reduce_mod(from_limbs28(&o[(size_t)i * 14])), sq ? want_sqr[i] : want_mul[i]) == 0;
                for (int q = 0; q < 13; q++) ok = ok && o[(size_t)i * 14 + q] <= M28;
                bad += !ok;
            }
            printf("# parity %s %-10s: %u mismatches on %u operand pairs (%zu x %zu edge pairs, the rest random)\n", sq ? "sqr" : "mul", FORM_NAME[f], bad, N, edge.size(), edge.size());
            bad_total += bad;
        }
    if (bad_total) { printf("PARITY FAILED\n"); return 2; }
    // ---- throughput: dependent chains, 1 / 2 / 4 waves per SIMD (256 workgroups of 4 W waves)
    Timing at2[2][N_FORMS] = {};
    for (int wps = 1; wps <= 4; wps *= 2) {
        printf("--- %d wave(s) per SIMD\n", wps);
        for (int sq = 0; sq < 2; sq++)
            for (int f = 0; f < N_FORMS; f++) {
                const launch_fn fn = sq ? SQR[f] : MUL[f];
                if (!fn) continue;
                const Timing tm = timed(sq ? "sqr" : "mul", FORM_NAME[f], wps, fn, d_in, d_out, d_st, N);
                if (wps == 2) at2[sq][f] = tm;
            }
    }
    // ---- the rule: a form replaces today's only if, at TWO waves per SIMD, its median beats a's by more than the spread of a's five launches
    for (int sq = 0; sq < 2; sq++) {
        const Timing a = at2[sq][F_PLAIN];
        int best = F_PLAIN;
        for (int f = 1; f < N_FORMS; f++) if ((sq ? SQR[f] : MUL[f]) && at2[sq][f].med < at2[sq][best].med) best = f;
        const bool wins = best != F_PLAIN && a.med - at2[sq][best].med > a.hi - a.lo;
        printf("# %s at 2 waves per SIMD: a-plain %.1f (spread %.1f); fastest %s %.1f (%+.2f %%): %s\n", sq ? "sqr" : "mul", a.med, a.hi - a.lo, FORM_NAME[best],
               at2[sq][best].med, 100.0 * (at2[sq][best].med - a.med) / a.med, wins ? "REPLACES a" : "a stays");
    }
    return 0;
}
