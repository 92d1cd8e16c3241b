// Pairing check, SIX LANES PER PROOF (ten proofs per wave): the engine for callers that keep the chip full anyway.
//
// Why: with the chip full the pairing kernel is bound by the issue rate of v_mad_u64_u32, so what counts is multiply-adds
// per pairing, not the length of the chain.  The one-coefficient-per-lane engine (h2v_pairing_coop.hpp, 16 lanes per proof)
// leaves 4 of 16 lanes idle outside the line steps, and a lane that owns ONE Fp coefficient of an Fp2 product has to
// take the schoolbook four products.  Here lane k < 6 of a group owns Fp2 coefficient k WHOLE, so
//   * 60 of 64 lanes work in every engine call (ten groups per wave), and
//   * an Fp2 x Fp2 term is a Karatsuba term - three Fp products into three sets of 64-bit column accumulators
//         U += x0 y0      V += x1 y1      W += (x0 + x1)(y0 + y1)        re = U - V      im = W - U - V
//     with ONE Montgomery reduction per part at the end of the call: (3 NT + 2) x 196 multiply-adds per Fp2 coefficient
//     where two lanes of the other engine spend 2 (2 NT + 1) x 196 (MUL, NT = 6: 3920 against 5096).
// The sums x0 + x1, y0 + y1 are formed LIMB-WISE in registers (uncarried), so W - U - V equals sum(x0 y1 + x1 y0) column by column: the
// imaginary part's columns are non-negative (unsigned reduction; W itself may wrap modulo 2^64 on the way - harmless);
// U - V is taken in two's complement columns (|column| < 2^63) and reduced with arithmetic carries, p added at the end.
// Wrapped terms (x xi) take the xi on the A side: XA = xi a = (a0 - a1, a0 + a1).  The cyclotomic squaring is four
// products into three sets (re = P1 + P2 - P4, im = P1 + P3 + P4: the set of P1 + P2 starts as a copy of P1's, taken as the
// addend of its first multiply-adds; six_csqr_products); the lane forms 3 r -/+ 2 g itself and folds it below 2p with a quotient
// estimate from the top limb (f28_fold).  A run of squarings - the hard part's x^|x| has runs of 1, 2, 3, 9, 32 and 16 between its
// multiplications - is ONE out-of-line call (six_csqr_run): the value stays in registers from one squaring's fold to the next one's
// staging.
// Miller lines have a UNIT coefficient: the plan's line c + ((-lambda) xP) w^2 + yP w^3 is divided by its own c (an Fp2 constant
// of the fixed G2 argument; any factor in Fp2* of the Miller value dies in the easy part of the final exponentiation), so
//   f (l / c) = f + f (a w^2 + b w^3),   a = A xP,  b = B yP,   A = -lambda / c,  B = 1 / c  (a table derived at plan load),
// is TWO Karatsuba terms per lane and the lane's own staged coefficient added after the reduction (8 units of 196 multiply-adds
// where the three-term line took 11).  Per round the eight products A_u xP_u, B_u yP_u (two parts each, both loops) are taken just
// before the line steps: six in one pass (one per lane), the last two in a second.  The value grows by the added coefficient
// from the squaring to the round's last line and falls back with the next squaring; the loop's staging takes re <= 12p,
// im <= 7p (gen_six_tables.py: miller_round_bounds), and the value is folded once after the loop.
// Tables and the headroom argument: tools/gen_six_tables.py (value-level check against big-integer Fp12 arithmetic and a
// limb-level model of this code with the column bounds asserted).  The device code is held to that model call by call: k_probe_six
// (below; h2v_probe_six_call) runs ONE engine call per group on raw limb vectors, and tests/test_six_engine_calls_gpu.py compares every
// result limb for limb with the model on operands at the stated bounds.  Program, line tables, semantics: h2v_pairing_coop.hpp.
//
// LDS: 38 operand slots of 56 bytes per proof (14 limbs, no padding: 8-byte reads), 23 KB per wave - six or seven waves per
// CU, and at most 256 registers per lane, so that a SIMD holds a second wave beside this one: a lone wave issues a
// v_mad_u64_u32 only every ~11 cycles, two waves one every ~5.5 (profiles/r03_imad_ubench.txt).  (A first version with staged
// sums and 80-byte slots - 47 KB per wave, 356 registers - was correct and 20 % SLOWER than the narrow engine in the full
// pipeline: 4.91 against 4.06 ms per step, the kernel alone 4.80 ms: its waves held their SIMDs alone.)
// Ten pairings share one instruction stream: for one batch at a time the other engines are faster; see launch_pairing.
#pragma once
#include "h2v_pairing_coop.hpp"
#include "six_tables.h"

#define H2V_NO_TAIL_MARK __attribute__((disable_tail_calls))
#define SIX_GROUPS 10
#define SIX_SLOT_DW 14
#define SIX_GROUP_DW (SIX_N_GROUP_SLOTS * SIX_SLOT_DW)
#define SIX_TAB_DW ((6 * 4 * SIX_N_MUL + 6 * 4 * SIX_N_SQR + 2 * 6 * 4 * SIX_N_LINE + 6 * 3 * SIX_N_CSQR) / 4)
#define SIX_TAB_OFF (SIX_N_SHARED_SLOTS * SIX_SLOT_DW)
#define SIX_GRP_OFF ((SIX_TAB_OFF + SIX_TAB_DW + 1) & ~1)
#define SIX_LDS_BYTES ((size_t)(SIX_GRP_OFF + SIX_GROUPS * SIX_GROUP_DW) * 4)
#define SIX_TAB_MUL_B 0
#define SIX_TAB_SQR_B (6 * 4 * SIX_N_MUL)
#define SIX_TAB_LINE1_B (SIX_TAB_SQR_B + 6 * 4 * SIX_N_SQR)
#define SIX_TAB_LINE2_B (SIX_TAB_LINE1_B + 6 * 4 * SIX_N_LINE)
#define SIX_TAB_CSQR_B (SIX_TAB_LINE2_B + 6 * 4 * SIX_N_LINE)
#define SIX_C_M(k) ((k) < 3 ? 19 + (k) : 31 + (k))      // gen_six_tables.py: C_M

struct Six {
    int grp_off;  // dword offset of the group's slots in coop_lds
    int k;        // Fp2 coefficient 0..5
    bool act;     // lanes 60..63 shadow group 9 and never store
};
struct SixF2 { F28 re, im; };
struct SixRegs { F28Regs re, im; };

H2V_DI int six_slot_dw(const Six &c, int s) {
    return s < SIX_SHARED_BASE ? c.grp_off + s * SIX_SLOT_DW : (s - SIX_SHARED_BASE) * SIX_SLOT_DW;
}
H2V_DI uint32_t *six_slot(const Six &c, int s) { return coop_lds + six_slot_dw(c, s); }
// ... of slot byte b of a table dword
H2V_DI uint32_t *six_slot_of(const Six &c, const uint32_t w, const int b) { return six_slot(c, (int)__builtin_amdgcn_ubfe(w, 8 * b, 8)); }
H2V_DI void six_store(uint32_t *p, const F28 &a) {   // limbs as staged (carried, or the doubled operands' 2^29)
    uint2 *q = reinterpret_cast<uint2 *>(p);
#pragma unroll
    for (int i = 0; i < 7; i++) q[i] = make_uint2(a.l[2 * i], a.l[2 * i + 1]);
}
H2V_DI void six_store(uint32_t *p, const Fp &a) {
    F28 t;
    f28_from_fp(t, a);
    six_store(p, t);
}
// Operand fetches of the squaring runs and the line products: ISSUE and ARRIVAL are separate steps, so that the reads of the NEXT
// operands are in flight while the 196 multiply-adds of the current product issue, and the wave meets their s_waitcnt after the
// product, when the data has long arrived.
// With every hot kernel at 248-256 registers a SIMD holds two waves, and while one of them sits in a wait the other issues
// v_mad_u64_u32 at half rate (profiles/r04_imad_ubench.txt).
//   six_issue    seven 64-bit LDS loads per operand (slots are 8-byte aligned 56-byte records), VOLATILE: they keep their place
//                among the pins below.  The waits stay the compiler's: it puts the s_waitcnt in front of the first instruction
//                that reads a fetched register, which is the arrival pin - no hand-written wait, nothing to get wrong when the
//                register allocator moves a fetched value.  (The asm block of coop_load28_pair answers the optimiser re-cutting
//                128-BIT loads; these are 64-bit and stay whole.)
//   six_arrive   an empty asm that reads and writes every register of two fetched operands: the compiler's wait stands in front of
//                it, no consumer of the operands is scheduled above it - and, given the CURRENT product's operands after the
//                issue of the next ones, that product cannot start above the issue.
//   six_done     an empty asm that reads and writes the 27 product columns of an accumulator set (column 27 holds no product and
//                stays a constant, not a register): the product cannot end below it.  Asm
//                statements and volatile loads keep their order, so  issue(next); arrive(current) ... product ... done(set);
//                arrive(next)  is what the wave executes.
// Program order is the one rule for correctness: the block is one wave and LDS executes in order, so a fetch may stand anywhere
// after the last store to its slot (and the barrier that publishes another lane's store) and before the next store to it.
struct SixOp { u32x2_t v[7]; };
H2V_DI void six_issue(SixOp &o, const uint32_t *p) {
    const volatile __attribute__((address_space(3))) u32x2_t *q = (const volatile __attribute__((address_space(3))) u32x2_t *)p;
#pragma unroll
    for (int i = 0; i < 7; i++) o.v[i] = q[i];
}
H2V_DI void six_arrive(SixOp &a, SixOp &b) {
    asm volatile(""
                 : "+v"(a.v[0]), "+v"(a.v[1]), "+v"(a.v[2]), "+v"(a.v[3]), "+v"(a.v[4]), "+v"(a.v[5]), "+v"(a.v[6]), "+v"(b.v[0]), "+v"(b.v[1]),
                   "+v"(b.v[2]), "+v"(b.v[3]), "+v"(b.v[4]), "+v"(b.v[5]), "+v"(b.v[6]));
}
H2V_DI void six_arrive(SixOp &a) {
    asm volatile("" : "+v"(a.v[0]), "+v"(a.v[1]), "+v"(a.v[2]), "+v"(a.v[3]), "+v"(a.v[4]), "+v"(a.v[5]), "+v"(a.v[6]));
}
H2V_DI void six_arrive(uint32_t (&a)[14], uint32_t (&b)[14]) {   // (limb sums: operands that were not fetched as they are)
    asm volatile(""
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]), "+v"(a[9]),
                   "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]),
                   "+v"(b[6]), "+v"(b[7]), "+v"(b[8]), "+v"(b[9]), "+v"(b[10]), "+v"(b[11]), "+v"(b[12]), "+v"(b[13]));
}
H2V_DI void six_done(uint64_t (&c)[28]) {
    asm volatile(""
                 : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]), "+v"(c[8]), "+v"(c[9]),
                   "+v"(c[10]), "+v"(c[11]), "+v"(c[12]), "+v"(c[13]), "+v"(c[14]), "+v"(c[15]), "+v"(c[16]), "+v"(c[17]), "+v"(c[18]),
                   "+v"(c[19]), "+v"(c[20]), "+v"(c[21]), "+v"(c[22]), "+v"(c[23]), "+v"(c[24]), "+v"(c[25]), "+v"(c[26]));
}
H2V_DI void six_limbs(uint32_t (&x)[14], const SixOp &o) {
#pragma unroll
    for (int i = 0; i < 7; i++) { x[2 * i] = o.v[i].x; x[2 * i + 1] = o.v[i].y; }
}
H2V_DI void six_load_pair(uint32_t (&x)[14], uint32_t (&y)[14], const uint32_t *px, const uint32_t *py) {   // fetched and waited for
    SixOp a, b;
    six_issue(a, px);
    six_issue(b, py);
    six_arrive(a, b);
    six_limbs(x, a);
    six_limbs(y, b);
}
H2V_DI void six_mac(uint64_t (&acc)[28], const uint32_t (&x)[14], const uint32_t (&y)[14]) {
#pragma unroll
    for (int i = 0; i < 14; i++)
#pragma unroll
        for (int j = 0; j < 14; j++) acc[i + j] += (uint64_t)x[i] * y[j];
}
// Montgomery reduction of 28 columns, R = 2^392.  SIGNED: two's complement columns, arithmetic carries, + p at the end
// (the value is above -p: gen_six_tables.py).  Result limbs carried.
template <bool SIGNED>
H2V_DI void six_reduce(F28 &r, uint64_t (&acc)[28]) {
#pragma unroll
    for (int k = 0; k < 14; k++) {
        const uint32_t m = ((uint32_t)acc[k] * FP_N0_28) & FP28_MASK;
#pragma unroll
        for (int j = 0; j < 14; j++) acc[k + j] += (uint64_t)m * FP_MOD28[j];
        acc[k + 1] += SIGNED ? (uint64_t)((int64_t)acc[k] >> 28) : acc[k] >> 28;
    }
    if (SIGNED) {
        int64_t carry = 0;
#pragma unroll
        for (int k = 0; k < 13; k++) {
            carry += (int64_t)acc[14 + k] + (int64_t)FP_MOD28[k];
            r.l[k] = (uint32_t)carry & FP28_MASK;
            carry >>= 28;
        }
        r.l[13] = (uint32_t)(carry + (int64_t)acc[27] + (int64_t)FP_MOD28[13]);
    } else {
        uint64_t carry = 0;
#pragma unroll
        for (int k = 0; k < 13; k++) {
            carry += acc[14 + k];
            r.l[k] = (uint32_t)carry & FP28_MASK;
            carry >>= 28;
        }
        r.l[13] = (uint32_t)(carry + acc[27]);
    }
}
// NT Karatsuba terms from the lane's table row (4 slot bytes per term: x0 y0 x1 y1) -> (re, im), both below 3p.
// addself (line steps): the lane's own staged coefficient (its A slots) is added to the result - as f R into columns 14..27
// before the reductions, whose final carry then serves both; the read comes before the write of the same slots below.
// The result does not come back through the call: it is written, carried, into the lane's own A slots (2k, 2k + 1) - every
// operand slot is dead once the last term has been read (one wave per block: the lanes have all read before any writes) -
// and the caller reads it from there (six_result).  A 28-dword struct is returned through private memory by the calling
// convention: a store, a wait for it, and a load per engine call, ~550 calls per pairing (round 3: the kernel's scratch
// traffic).  keep (per lane): leave the A slots as they are - the staged input survives (line steps of a skipped loop).
// The term loop fetches where it uses (six_load_pair): with three accumulator sets and two operand pairs live it is the one place
// without registers for operands in flight - see DESIGN 4.1.1 for what the overlapped form of this loop cost and measured.
H2V_DN void six_kara(const Six c, const int tab_row_byte, const int nt, const bool keep, const bool addself) {
    const uint8_t *tab = reinterpret_cast<const uint8_t *>(coop_lds + SIX_TAB_OFF) + tab_row_byte;
    uint64_t U[28], V[28], W[28];
#pragma unroll
    for (int i = 0; i < 28; i++) { U[i] = 0; V[i] = 0; W[i] = 0; }
#pragma unroll 1
    for (int t = 0; t < nt; t++) {
        uint32_t x0[14], y0[14], x1[14], y1[14];
        six_load_pair(x0, y0, six_slot(c, tab[4 * t]), six_slot(c, tab[4 * t + 1]));
        six_mac(U, x0, y0);
        six_load_pair(x1, y1, six_slot(c, tab[4 * t + 2]), six_slot(c, tab[4 * t + 3]));
        six_mac(V, x1, y1);
#pragma unroll
        for (int i = 0; i < 14; i++) { x1[i] += x0[i]; y1[i] += y0[i]; }
        six_mac(W, x1, y1);
    }
#pragma unroll
    for (int i = 0; i < 27; i++) {   // (column 27 holds no product)
        W[i] -= U[i] + V[i];
        U[i] -= V[i];
    }
    if (addself) {
        uint32_t f0[14], f1[14];
        six_load_pair(f0, f1, six_slot(c, SIX_SLOT_A + 2 * c.k), six_slot(c, SIX_SLOT_A + 2 * c.k + 1));
#pragma unroll
        for (int i = 0; i < 14; i++) { U[14 + i] += f0[i]; W[14 + i] += f1[i]; }
    }
    SixF2 r;
    six_reduce<false>(r.im, W);
    six_reduce<true>(r.re, U);
    if (c.act && !keep) {
        six_store(six_slot(c, SIX_SLOT_A + 2 * c.k), r.re);
        six_store(six_slot(c, SIX_SLOT_A + 2 * c.k + 1), r.im);
    }
}
// an engine's result (or a staged value) back from the lane's slots `base + 2k`, `base + 2k + 1`; shadow lanes read group 9's
H2V_DI SixF2 six_result(const Six &c, const int base) {
    SixF2 r;
    six_load_pair(r.re.l, r.im.l, six_slot(c, base + 2 * c.k), six_slot(c, base + 2 * c.k + 1));
    return r;
}
// acc2 = acc + x y, acc2 not yet written: the first multiply-add into each column of acc2 (row 0 and the last of every other
// row) takes acc's column as its addend - v_mad_u64_u32 writes D = S0 S1 + S2 with D apart from S2, so the copy costs nothing.
H2V_DI void six_mac_from(uint64_t (&acc2)[28], const uint64_t (&acc)[28], const uint32_t (&x)[14], const uint32_t (&y)[14]) {
#pragma unroll
    for (int i = 0; i < 14; i++)
#pragma unroll
        for (int j = 0; j < 14; j++) acc2[i + j] = ((i == 0 || j == 13) ? acc[i + j] : acc2[i + j]) + (uint64_t)x[i] * y[j];
}
// cyclotomic squaring: four products (x + x2) y, P1..P4 (3 slot bytes each; gen_six_tables.py: csqr_table), into three sets
//   A = P1     B = A + P2 (B starts as a copy of A)     A += P3     C = P4     ->  re = B - C (signed columns), im = A + C,
// reduced: re below 2.2p, im below 1.2p.  The lane finishes with 3 r -/+ 2 g (six_csqr_run).
// Fetch schedule (see six_issue): the whole triple of product T + 1 goes under product T - B is not live before P2 and C not before
// P4, so under P3 the count is two sets, x, y and the next triple - and the read-back of g (the lane's A slots; x itself is not
// kept in registers while the three sets are live) under the two reductions.  tw: the row's 12 table bytes as three dwords, read
// once per run by the caller.
H2V_DI const uint32_t *six_csqr_slot(const Six &c, const uint32_t (&tw)[3], const int b) {
    return six_slot_of(c, tw[b >> 2], b & 3);
}
H2V_DI void six_csqr_products(const Six &c, const uint32_t (&tw)[3], SixF2 &r, SixF2 &g) {
    uint64_t A[28], B[28], C[28];
#pragma unroll
    for (int i = 0; i < 28; i++) { A[i] = 0; C[i] = 0; }
    B[27] = 0;                       // (column 27 holds no product)
    uint32_t x[14], y[14], x2[14];
    SixOp fx, fx2, fy;
#define SIX_CSQR_ISSUE(T)                                                                                \
    do {                                                                                                 \
        six_issue(fx, six_csqr_slot(c, tw, 3 * (T)));                                                    \
        six_issue(fx2, six_csqr_slot(c, tw, 3 * (T) + 1));                                               \
        six_issue(fy, six_csqr_slot(c, tw, 3 * (T) + 2));                                                \
    } while (0)
#define SIX_CSQR_TAKE()                                                                                  \
    do {                                                                                                 \
        six_arrive(fx, fx2);                                                                             \
        six_arrive(fy);                                                                                  \
        six_limbs(x, fx);                                                                                \
        six_limbs(x2, fx2);                                                                              \
        six_limbs(y, fy);                                                                                \
        _Pragma("unroll") for (int i_ = 0; i_ < 14; i_++) x[i_] += x2[i_];                               \
    } while (0)
    SIX_CSQR_ISSUE(0);
    SIX_CSQR_TAKE();
    SIX_CSQR_ISSUE(1);
    six_arrive(x, y);
    six_mac(A, x, y);
    six_done(A);
    SIX_CSQR_TAKE();
    SIX_CSQR_ISSUE(2);
    six_arrive(x, y);
    six_mac_from(B, A, x, y);
    six_done(B);
    SIX_CSQR_TAKE();
    SIX_CSQR_ISSUE(3);
    six_arrive(x, y);
    six_mac(A, x, y);
    six_done(A);
    SIX_CSQR_TAKE();
    six_mac(C, x, y);
#undef SIX_CSQR_ISSUE
#undef SIX_CSQR_TAKE
    six_done(C);
    six_issue(fx, six_slot(c, SIX_SLOT_A + 2 * c.k));
    six_issue(fy, six_slot(c, SIX_SLOT_A + 2 * c.k + 1));
    six_done(B);                     // (the reductions start below the issue)
    six_done(A);
#pragma unroll
    for (int i = 0; i < 27; i++) {
        B[i] -= C[i];
        A[i] += C[i];
    }
    six_reduce<true>(r.re, B);
    six_reduce<false>(r.im, A);
    six_arrive(r.re.l, r.im.l);   // (the reductions end above g's arrival)
    six_arrive(fx, fy);
    six_limbs(g.re.l, fx);
    six_limbs(g.im.l, fy);
}
// A RUN of n cyclotomic squarings as one call: the value comes in and goes back through the lane's A slots (staged by the caller,
// read by six_result), and between two squarings of the run it stays in registers - per squaring: staging (D = 2x into the B slots,
// M into its slot; x itself is in the A slots already), the four products and two reductions, h = 3 r -/+ 2 g, the fold, and x back
// into the A slots, which is both the next squaring's staging and the run's result.  g is read back from the A slots after the
// products (nothing of x stays live while the three accumulator sets are).  Barriers as around every engine call: after the
// staging, and after the last read (the lane's own g) before any lane writes again.  The next squaring's first fetch stands after
// the barrier that follows its staging: it reads what this one's A-slot store and that staging wrote.
H2V_DN void six_csqr_run(const Six c, const int tab_row_byte, const int n) {
    static_assert(SIX_TAB_CSQR_B % 4 == 0 && SIX_N_CSQR == 4, "a row of the squaring's table is three dwords");
    const uint32_t *tabw = coop_lds + SIX_TAB_OFF + (tab_row_byte >> 2);
    const uint32_t tw[3] = {tabw[0], tabw[1], tabw[2]};
    SixF2 x = six_result(c, SIX_SLOT_A);
    const bool minus = (c.k & 1) == 0;
#pragma unroll 1
    for (int rep = 0; rep < n; rep++) {
        if (c.act) {
            F28 d0, d1, m;
            F28_SUB(m, x.re, x.im, 7, 1);          // M = re - im + 7p                         (13, 4)
            f28_carry(m);
            f28_mul_small<2>(d0, x.re);            // D = 2x, uncarried                        (12, 2)
            f28_mul_small<2>(d1, x.im);
            six_store(six_slot(c, SIX_SLOT_B + 2 * c.k), d0);
            six_store(six_slot(c, SIX_SLOT_B + 2 * c.k + 1), d1);
            six_store(six_slot(c, SIX_C_M(c.k)), m);
        }
        __syncthreads();
        SixF2 r, g;
        six_csqr_products(c, tw, r, g);
        // h_k = 3 Q_k - 2 g_k (k even) / + 2 g_k (k odd), folded: 3 r + (13p - 2g | 2g) is below 20p (r < 2.2p, g < 6p), the fold
        // brings it below 2p.  (The other engines multiply g by the constants -/+ 2/3 inside the sum: two products more per lane.)
        // The sum goes to the fold UNCARRIED (limbs below 2^31): the fold's own signed carry chain normalises the limbs, and its
        // quotient estimate from the uncarried top limb is short of the carried one's by the carry the lower limbs would have sent
        // up (at most 7 against p's top limb near 2^24.7) - still never too large, still at most one too small
        // (gen_six_tables.py: fold, checked with every lower limb at its maximum).
#pragma unroll
        for (int i = 0; i < 14; i++) {
            const uint32_t g0 = g.re.l[i] << 1, g1 = g.im.l[i] << 1;
            x.re.l[i] = 3u * r.re.l[i] + (minus ? F28_BIAS_13_2[i] - g0 : g0);
            x.im.l[i] = 3u * r.im.l[i] + (minus ? F28_BIAS_13_2[i] - g1 : g1);
        }
        f28_fold(x.re);
        f28_fold(x.im);
        __syncthreads();
        if (c.act) {
            six_store(six_slot(c, SIX_SLOT_A + 2 * c.k), x.re);
            six_store(six_slot(c, SIX_SLOT_A + 2 * c.k + 1), x.im);
        }
    }
}
// The line products of a Miller round as one call: x1 y1 into the lane's T slot, x2 y2 into T slot 6 + k of lanes 0 and 1, each
// reduced (< 2p).  Both operand pairs are fetched up front (one accumulator set is live: registers are plentiful), so the second
// product meets no wait.  No operand is a T slot.
H2V_DN void six_prod2(const Six c, const int xs1, const int ys1) {
    const int xs2 = SIX_SLOT_LN2 + 2 + (c.k & 1), ys2 = SIX_SLOT_PY2;     // (lanes 0, 1: the parts of b of loop 2)
    SixOp fx, fy, fx2, fy2;
    six_issue(fx, six_slot(c, xs1));
    six_issue(fy, six_slot(c, ys1));
    six_issue(fx2, six_slot(c, xs2));
    six_issue(fy2, six_slot(c, ys2));
    six_arrive(fx, fy);
    uint32_t x[14], y[14];
    F28 r;
    {
        uint64_t acc[28];
#pragma unroll
        for (int i = 0; i < 28; i++) acc[i] = 0;
        six_limbs(x, fx);
        six_limbs(y, fy);
        six_mac(acc, x, y);
        six_reduce<false>(r, acc);
    }
    if (c.act) six_store(six_slot(c, SIX_SLOT_T + c.k), r);
    six_arrive(fx2, fy2);
    {
        uint64_t acc[28];
#pragma unroll
        for (int i = 0; i < 28; i++) acc[i] = 0;
        six_limbs(x, fx2);
        six_limbs(y, fy2);
        six_mac(acc, x, y);
        six_reduce<false>(r, acc);
    }
    if (c.act && c.k < 2) six_store(six_slot(c, SIX_SLOT_T + 6 + c.k), r);
}
H2V_DI SixF2 six_unpack(const SixRegs &z) {
    SixF2 r;
    r.re = f28_unpack(z.re.a, z.re.b, z.re.c, z.re.d);
    r.im = f28_unpack(z.im.a, z.im.b, z.im.c, z.im.d);
    return r;
}

// ---- staging (values: v <= 6, carried; MILLER - the loop's squaring and lines - re <= 12p, im <= 7p).  Slots: six_tables.h / gen_six_tables.py
template <bool MILLER = false>
H2V_DI void six_stage_a(const Six &c, const SixF2 &a, const int xa_from) {
    if (!c.act) return;
    six_store(six_slot(c, SIX_SLOT_A + 2 * c.k), a.re);
    six_store(six_slot(c, SIX_SLOT_A + 2 * c.k + 1), a.im);
    if (c.k >= xa_from) {   // xi a = (re - im + 7p, re + im); in the Miller loop + 11p (SIX_MILLER_K)
        F28 t, x0, x1;
        static_assert(SIX_MILLER_K == 11, "the bias table of the Miller loop's staging");
        if (MILLER) F28_NEG(t, a.im, 11, 1);
        else F28_NEG(t, a.im, 7, 1);
        f28_add(x0, a.re, t);
        f28_carry(x0);
        f28_add(x1, a.re, a.im);
        f28_carry(x1);
        six_store(six_slot(c, SIX_SLOT_XA + 2 * (c.k - 1)), x0);
        six_store(six_slot(c, SIX_SLOT_XA + 2 * (c.k - 1) + 1), x1);
    }
}
H2V_DI void six_stage_b(const Six &c, const SixF2 &b) {
    if (!c.act) return;
    six_store(six_slot(c, SIX_SLOT_B + 2 * c.k), b.re);
    six_store(six_slot(c, SIX_SLOT_B + 2 * c.k + 1), b.im);
}
H2V_DI void six_stage_d(const Six &c, const SixF2 &a) {   // D = 2a, uncarried
    if (!c.act) return;
    F28 d0, d1;
    f28_mul_small<2>(d0, a.re);
    f28_mul_small<2>(d1, a.im);
    six_store(six_slot(c, SIX_SLOT_B + 2 * c.k), d0);
    six_store(six_slot(c, SIX_SLOT_B + 2 * c.k + 1), d1);
}
H2V_DI SixF2 six_mul(const Six &c, const SixF2 &a, const SixF2 &b) {
    six_stage_a(c, a, 1);
    six_stage_b(c, b);
    __syncthreads();
    six_kara(c, SIX_TAB_MUL_B + c.k * 4 * SIX_N_MUL, SIX_N_MUL, false, false);
    __syncthreads();
    return six_result(c, SIX_SLOT_A);
}
H2V_DI SixF2 six_sqr(const Six &c, const SixF2 &a) {   // (the Miller loop's squaring)
    six_stage_a<true>(c, a, 3);
    six_stage_d(c, a);
    __syncthreads();
    six_kara(c, SIX_TAB_SQR_B + c.k * 4 * SIX_N_SQR, SIX_N_SQR, false, false);
    __syncthreads();
    return six_result(c, SIX_SLOT_A);
}
// f times the unit-coefficient line of loop LOOP; skip (per proof: that loop's G1 argument is infinity): f comes back unchanged
template <int LOOP>
H2V_DI SixF2 six_line(const Six &c, const SixF2 &f, const bool skip) {
    six_stage_a<true>(c, f, 3);
    __syncthreads();
    six_kara(c, (LOOP == 1 ? SIX_TAB_LINE1_B : SIX_TAB_LINE2_B) + c.k * 4 * SIX_N_LINE, SIX_N_LINE, skip, true);
    __syncthreads();
    return six_result(c, SIX_SLOT_A);
}
H2V_DI SixF2 six_csqr(const Six &c, const SixF2 &a, const int n) {   // a^(2^n), a in the cyclotomic subgroup
    if (c.act) {
        six_store(six_slot(c, SIX_SLOT_A + 2 * c.k), a.re);
        six_store(six_slot(c, SIX_SLOT_A + 2 * c.k + 1), a.im);
    }
    __syncthreads();
    six_csqr_run(c, SIX_TAB_CSQR_B + c.k * 3 * SIX_N_CSQR, n);
    __syncthreads();
    return six_result(c, SIX_SLOT_A);
}
H2V_DI SixF2 six_conj(const Six &c, const SixF2 &a) {   // w -> -w: odd coefficients change sign.  a: v <= 5
    SixF2 r = a;
    if (c.k & 1) {
        F28_NEG(r.re, a.re, 6, 1);
        F28_NEG(r.im, a.im, 6, 1);
        f28_carry(r.re);
        f28_carry(r.im);
    }
    return r;
}
H2V_DI SixF2 six_frob(const Six &c, const SixF2 &a) {   // a -> a^p: coefficient k becomes conj(a_k) * gamma^k.  Result v <= 5
    Fp g0, g1;
#pragma unroll
    for (int i = 0; i < 12; i++) { g0.v[i] = FROB_GAMMA[c.k][0][i]; g1.v[i] = FROB_GAMMA[c.k][1][i]; }
    F28 h0, h1, x, y;
    f28_from_fp(h0, g0);
    f28_from_fp(h1, g1);
    SixF2 r;
    f28_mul(x, a.re, h0); f28_mul(y, a.im, h1); f28_add(r.re, x, y);          // re g0 + im g1
    f28_mul(x, a.re, h1); f28_mul(y, a.im, h0); F28_SUB(r.im, x, y, 3, 1);    // re g1 - im g0
    f28_carry(r.re);
    f28_carry(r.im);
    return r;
}
// 1/f = conj(f) / N with N = f conj(f) in Fp6 (the even coefficients).  1/N without tower code on one lane: the conjugates of
// N over Fp2 are its images under Frobenius p^2 and p^4, so adj = N^(p^2) N^(p^4) and N adj = Norm(N) lies in Fp2 (coefficient 0);
// lane 0 of the group inverts that one Fp2 element (one Fp inversion), and 1/N = adj / Norm(N).  Four Frobenius maps and four
// engine products more than the tower inversion the other engines run on their first lane - and 1.2 KB less scratch per lane
// (Fp6 temporaries and the frames of fp6_inv), which is what a queue's scratch arena is sized by.
// (H2V_NO_TAIL_MARK: see k_pairing_six)
H2V_DN H2V_NO_TAIL_MARK SixRegs six_inv_raw(const Six c, const SixRegs fr, bool &ok) {
    const SixF2 f = six_unpack(fr);
    const SixF2 fc = six_conj(c, f);
    const SixF2 nrm = six_mul(c, f, fc);                       // N
    const SixF2 n2 = six_frob(c, six_frob(c, nrm));            // N^(p^2)        (v <= 5)
    const SixF2 n4 = six_frob(c, six_frob(c, n2));             // N^(p^4)
    const SixF2 adj = six_mul(c, n2, n4);
    const SixF2 nn = six_mul(c, nrm, adj);                     // Norm(N): coefficient 0 only
    Fp2 z, zi;
    f28_to_fp(z.c0, nn.re);
    f28_to_fp(z.c1, nn.im);
    fp_set_zero(zi.c0);
    fp_set_zero(zi.c1);
    bool good = true;
    if (c.k == 0) good = fp2_inv(zi, z);
    ok = good;
    SixF2 ninv;                                                // 1 / Norm(N) as an Fp12 element: coefficient 0, zero elsewhere
    f28_from_fp(ninv.re, zi.c0);
    f28_from_fp(ninv.im, zi.c1);
    const SixF2 r = six_mul(c, fc, six_mul(c, adj, ninv));
    SixRegs o;
    o.re = f28_pack(r.re);
    o.im = f28_pack(r.im);
    return o;
}
// The constants of line `idx` of BOTH loops as the lane's share of the copy into the wave-shared slots: 2 x 4 slots
// [A0, A1, B0, B1] x 16 dwords in the plan-load table (14 limbs + 2 of padding), lane -> slot lane / 8, dwords 2 (lane % 8)..
H2V_DI uint2 six_line_share(const uint32_t *norm28, int idx, int lane) {
    return reinterpret_cast<const uint2 *>(norm28 + (size_t)idx * 8 * 16)[lane];
}
H2V_DI void six_line_store(const uint2 v, int lane) {
    static_assert(SIX_SLOT_LN2 == SIX_SLOT_LN1 + 4, "the two loops' constants are one run of eight slots");
    if ((lane & 7) == 7) return;    // the padding
    uint32_t *dst = coop_lds + (SIX_SLOT_LN1 - SIX_SHARED_BASE + (lane >> 3)) * SIX_SLOT_DW + 2 * (lane & 7);
    dst[0] = v.x;
    dst[1] = v.y;
}

// What every kernel of this engine starts with (k_pairing_six, and k_probe_six, which runs single engine calls for the tests):
// the lane's place - ten groups of six lanes, lanes 60..63 shadowing group 9 - (returns the group), and the operand tables and
// the shared zero operand in LDS.  The callers' first barrier publishes both.
H2V_DI int six_lane_setup(Six &c, const int lane) {
    const int grp6 = (lane * 43) >> 8;          // lane / 6 for lane < 64
    c.act = lane < 6 * SIX_GROUPS;
    const int grp = c.act ? grp6 : SIX_GROUPS - 1;
    c.k = c.act ? lane - 6 * grp6 : lane - 6 * SIX_GROUPS;
    c.grp_off = SIX_GRP_OFF + grp * SIX_GROUP_DW;
    return grp;
}
H2V_DI void six_tables_to_lds(const int lane) {
    {   // operand tables -> LDS
        const uint32_t *src[5] = {reinterpret_cast<const uint32_t *>(&SIX_TAB_MUL[0][0]), reinterpret_cast<const uint32_t *>(&SIX_TAB_SQR[0][0]),
                                  reinterpret_cast<const uint32_t *>(&SIX_TAB_LINE1[0][0]), reinterpret_cast<const uint32_t *>(&SIX_TAB_LINE2[0][0]),
                                  reinterpret_cast<const uint32_t *>(&SIX_TAB_CSQR[0][0])};
        const int off[6] = {SIX_TAB_MUL_B / 4, SIX_TAB_SQR_B / 4, SIX_TAB_LINE1_B / 4, SIX_TAB_LINE2_B / 4, SIX_TAB_CSQR_B / 4, SIX_TAB_DW};
#pragma unroll
        for (int t = 0; t < 5; t++)
            for (int q = lane; q < off[t + 1] - off[t]; q += 64) coop_lds[SIX_TAB_OFF + off[t] + q] = src[t][q];
    }
    if (lane < 14) coop_lds[(SIX_SLOT_ZERO - SIX_SHARED_BASE) * SIX_SLOT_DW + lane] = 0u;   // the shared zero operand
}
// The first pass of six_prod2 by lane: lane k < 4 takes part k & 1 of a = A xP of loop 1 + (k >> 1), lanes 4, 5 the parts of
// b = B yP of loop 1 (the second pass, lanes 0 and 1, those of b of loop 2: six_prod2 itself).  Macros, not a function: six_prod2 is
// compiled for the slot ranges its call sites hand it (an x operand in a shared slot, a y operand in the group's: six_slot_dw's
// choice is then made at compile time), and that analysis runs before any function is inlined - it has to see constants here.
#define SIX_PROD2_XS1(k) ((k) < 4 ? ((((k) >> 1) & 1) ? SIX_SLOT_LN2 : SIX_SLOT_LN1) + ((k) & 1) : SIX_SLOT_LN1 + 2 + ((k) & 1))
#define SIX_PROD2_YS1(k) ((k) < 4 ? ((((k) >> 1) & 1) ? SIX_SLOT_PX2 : SIX_SLOT_PX1) : SIX_SLOT_PY1)

// The engines return nothing and take no pointer into their caller's frame, so LLVM would mark their call sites `tail`; a
// callee with a `tail`-marked call site is excluded from the interprocedural register allocation's no-callee-saved-registers
// form (TargetFrameLowering::isSafeForNoCSROpt), and six_kara - which uses every register - would save and restore all 112
// callee-saved VGPRs through private memory on every call (seen: 106 stores + 106 loads per call).  The callers therefore
// opt out of tail-call marking.
extern "C" __global__ void __launch_bounds__(64, 2) H2V_NO_TAIL_MARK
k_pairing_six(H2vDevPlan plan, uint32_t n, const uint32_t *__restrict__ pts, const uint8_t *__restrict__ valid, const uint8_t *__restrict__ valid_sub,
              const uint32_t *__restrict__ er_jac, const uint32_t *__restrict__ el_jac /* folded el (recursion) or NULL */,
              uint32_t *__restrict__ status, uint8_t *__restrict__ accept, uint32_t *__restrict__ dbg) {
    const int lane = threadIdx.x;
    Six c;
    const int grp = six_lane_setup(c, lane);
    const int leader = grp * 6;
    const bool is_leader = c.act && c.k == 0;
    const uint32_t i = blockIdx.x * SIX_GROUPS + grp;
    const bool live = i < n;
    const uint32_t ii = live ? i : n - 1;       // dead groups shadow the last proof, never write
    const uint32_t slots = H2V_SLOTS(plan);

    six_tables_to_lds(lane);
    // ---- leader: status, the two G1 arguments (el ; -er normalised to affine)
    uint32_t st = 0;
    uint32_t flags = 0;  // bit0: el is infinity, bit1: er is infinity
    if (is_leader) {
        st = status[ii];
        for (uint32_t j = 0; j < slots; j++)
            if (!valid[(size_t)ii * slots + j] || (valid_sub && !valid_sub[(size_t)ii * slots + j])) st |= H2V_ST_BAD_POINT;
        G1A el, er;
        G1J ej;
        const uint32_t *pp = pts + ((size_t)ii * slots + plan.pi_point) * 24;
#pragma unroll
        for (int q = 0; q < 12; q++) {
            el.x.v[q] = pp[q]; el.y.v[q] = pp[12 + q];
            ej.x.v[q] = er_jac[(size_t)ii * 36 + q]; ej.y.v[q] = er_jac[(size_t)ii * 36 + 12 + q]; ej.z.v[q] = er_jac[(size_t)ii * 36 + 24 + q];
        }
        if (st != 0) { g1a_set_inf(el); g1j_set_inf(ej); }  // rejected already: keep the arithmetic well-defined
        g1j_to_affine(er, ej);
        if (el_jac && st == 0) {
            G1J lj;
#pragma unroll
            for (int q = 0; q < 12; q++) { lj.x.v[q] = el_jac[(size_t)ii * 36 + q]; lj.y.v[q] = el_jac[(size_t)ii * 36 + 12 + q]; lj.z.v[q] = el_jac[(size_t)ii * 36 + 24 + q]; }
            g1j_to_affine(el, lj);
        }
        if (g1a_is_inf(el)) flags |= 1;
        if (g1a_is_inf(er)) flags |= 2;
        fp_neg(er.y, er.y);
        six_store(six_slot(c, SIX_SLOT_PX1), el.x);
        six_store(six_slot(c, SIX_SLOT_PY1), el.y);
        six_store(six_slot(c, SIX_SLOT_PX2), er.x);
        six_store(six_slot(c, SIX_SLOT_PY2), er.y);
    }
    flags = __shfl(flags, leader);
    st = __shfl(st, leader);
    const bool skip1 = (flags & 1) != 0, skip2 = (flags & 2) != 0;
    bool inv_ok = true;
    __syncthreads();

    SixF2 vars[COOP_N_VARS];
    for (int pc = 0; pc < COOP_PROGRAM_LEN; pc++) {
        const uint32_t ins = COOP_PROGRAM[pc];
        const int op = ins & 0xff, d = (ins >> 8) & 0xff, a = (ins >> 16) & 0xff, b = ins >> 24;
        if (op == COOP_OP_END) break;
        switch (op) {
        case COOP_OP_MUL: {
            const SixF2 x = vars[a], y = vars[b];
            vars[d] = six_mul(c, x, y);
        } break;
        case COOP_OP_CSQR: {
            const SixF2 x = vars[a];
            vars[d] = six_csqr(c, x, b);
        } break;
        case COOP_OP_MILLER: {
            // Per bit of |x| below the leading one: F = F^2, then one or two rounds of { the products a = A xP, b = B yP of both
            // loops' lines: lane k < 4 takes part k & 1 of a of loop 1 + (k >> 1), lanes 4, 5 the parts of b of loop 1, and a second
            // pass (lanes 0, 1) those of b of loop 2; line of loop 1, line of loop 2 }.  The constants of the next round's
            // two lines are fetched a round ahead into one register pair per lane.
            SixF2 f = vars[COOP_VAR_F];
            int ln = 0;
            uint2 cn = six_line_share(plan.six_norm28, 0, lane);
            const int xs1 = SIX_PROD2_XS1(c.k), ys1 = SIX_PROD2_YS1(c.k);
#pragma unroll 1
            for (int bit = 62; bit >= 0; bit--) {
                f = six_sqr(c, f);
                const int steps = ((BLS_X_ABS >> bit) & 1) ? 2 : 1;
#pragma unroll 1
                for (int s2 = 0; s2 < steps; s2++, ln++) {
                    six_line_store(cn, lane);
                    if (ln + 1 < H2V_MILLER_LINES) cn = six_line_share(plan.six_norm28, ln + 1, lane);
                    __syncthreads();
                    six_prod2(c, xs1, ys1);
                    f = six_line<1>(c, f, skip1);                   // (its staging barrier also covers the T slots)
                    f = six_line<2>(c, f, skip2);
                }
            }
            f28_fold(f.re);                                         // (below 12p, 7p -> below 2p and a hair: what the program's
            f28_fold(f.im);                                         //  CONJ / INV / MUL take)
            vars[COOP_VAR_F] = f;
        } break;
        case COOP_OP_EXPX: {   // d = a^x (x < 0: conjugate of a^|x|)
            SixF2 x = vars[a];
            int run = 0;               // squarings since the last multiplication: runs of 1, 2, 3, 9, 32 and 16
#pragma unroll 1
            for (int bit = 62; bit >= 0; bit--) {
                run++;
                const bool set = ((BLS_X_ABS >> bit) & 1) != 0;
                if (!set && bit != 0) continue;
                x = six_csqr(c, x, run);
                run = 0;
                if (set) {
                    const SixF2 y = vars[a];
                    x = six_mul(c, x, y);
                }
            }
            vars[d] = six_conj(c, x);
        } break;
        case COOP_OP_WARMUP: break;   // (the other engines' first-line products: here every round takes its own)
        case COOP_OP_CONJ: vars[d] = six_conj(c, vars[a]); break;
        case COOP_OP_FROB: vars[d] = six_frob(c, vars[a]); break;
        case COOP_OP_INV: {
            bool ok = true;
            SixRegs fr;
            fr.re = f28_pack(vars[a].re);
            fr.im = f28_pack(vars[a].im);
            vars[d] = six_unpack(six_inv_raw(c, fr, ok));
            inv_ok = ok;
        } break;
        case COOP_OP_MOV: vars[d] = vars[a]; break;
        case COOP_OP_SETONE: {
            SixF2 o;
            f28_set_zero(o.re);
            f28_set_zero(o.im);
            if (c.k == 0) f28_set_one(o.re);
            vars[d] = o;
        } break;
        case COOP_OP_DUMP: {
            if (dbg && live && c.act) {
                Fp2 v;
                f28_to_fp(v.c0, vars[a].re);
                f28_to_fp(v.c1, vars[a].im);
                if (d == 0) {
                    // dump 0 is the Miller value.  With unit-coefficient lines it is the plan's Miller value divided by the
                    // product K of the lines' c along the loop's schedule (an Fp2 constant per loop, coefficient w^0: the
                    // conjugation leaves it alone); the probe reports the plan's value, so K goes back in HERE - the verdict's path
                    // never touches it.  six_k: [1, K1, K2, K1 K2] by the proof's skip flags (a skipped loop has no lines).
                    const uint32_t *kp = plan.six_k + ((skip1 ? 0 : 1) + (skip2 ? 0 : 2)) * 24;
                    Fp2 kk, t;
#pragma unroll
                    for (int q = 0; q < 12; q++) { kk.c0.v[q] = kp[q]; kk.c1.v[q] = kp[12 + q]; }
                    fp2_mul(t, v, kk);
                    v = t;
                }
                Fp o;
                fp_from_mont(o, v.c0);
#pragma unroll
                for (int q = 0; q < 12; q++) dbg[((size_t)i * 24 + 12 * d + 2 * c.k) * 12 + q] = o.v[q];
                fp_from_mont(o, v.c1);
#pragma unroll
                for (int q = 0; q < 12; q++) dbg[((size_t)i * 24 + 12 * d + 2 * c.k + 1) * 12 + q] = o.v[q];
            }
        } break;
        default: break;
        }
    }
    // == 1 ?
    Fp res0, res1;
    f28_to_fp(res0, vars[COOP_VAR_F].re);
    f28_to_fp(res1, vars[COOP_VAR_F].im);
    bool mine = fp_is_zero(res1);
    if (c.k == 0) { Fp one; fp_set_one(one); mine = mine && fp_eq(res0, one); }
    else mine = mine && fp_is_zero(res0);
    const unsigned long long bal = __ballot(mine);
    const bool is_one = ((bal >> leader) & 0x3full) == 0x3full;
    inv_ok = __shfl((int)inv_ok, leader) != 0;
    if (is_leader && live) {
        if (st == 0 && !(is_one && inv_ok)) st |= H2V_ST_PAIRING;
        status[i] = st;
        accept[i] = st == 0 ? 1 : 0;
    }
}

// ---- dev probe: ONE engine call per group, on raw limb vectors, through the functions the pairing calls (h2v_probe_six_call;
// tests/test_six_engine_calls_gpu.py holds every result to the limb model of tools/gen_six_tables.py, limb for limb, with the
// operands ON the bounds the headroom argument states).  Launch as k_pairing_six's: one wave per block, ten groups, lanes 60..63
// shadowing group 9, SIX_LDS_BYTES of dynamic LDS; a dead group shadows the last live one and writes nothing.
//   a, b      n x 12 vectors of 14 dwords: parts (re, im) of coefficients 0..5, as the lane stages them (carried, or for FOLD not)
//             b: MUL's second operand; LINE1 / LINE2: vectors 0..7 are the T slots 22..29; else unread
//   pts       n x 4 vectors: the point slots PX1, PY1, PX2, PY2 (PROD2, ROUND)
//   flags     n words: bit 0 skip1, bit 1 skip2 (LINE1, LINE2, ROUND)
//   lines16   the constants of one line of both loops as the plan-load table has them: 8 slots [A0, A1, B0, B1] x 2 of 16 dwords
//             (14 limbs and 2 of padding), copied into the wave-shared slots by six_line_share / six_line_store (PROD2, ROUND)
//   out       n x 6 x 28 dwords, lane k of group i at (6 i + k) 28: what six_result yields, re then im.  PROD2: the group's slots
//             22..29 at 168 i + 14 j instead.        ok_out    n words, INV alone: the leader's `ok`
#define SIX_PROBE_MUL 0
#define SIX_PROBE_SQR 1
#define SIX_PROBE_LINE1 2
#define SIX_PROBE_LINE2 3
#define SIX_PROBE_PROD2 4
#define SIX_PROBE_ROUND 5
#define SIX_PROBE_CSQR 6
#define SIX_PROBE_CONJ 7
#define SIX_PROBE_FROB 8
#define SIX_PROBE_INV 9
#define SIX_PROBE_FOLD 10
#define SIX_PROBE_N_OPS 11
#define SIX_PROBE_OUT_DW (6 * 2 * SIX_SLOT_DW)
H2V_DI void six_probe_vec(F28 &r, const uint32_t *__restrict__ src, const size_t vec) {
#pragma unroll
    for (int q = 0; q < SIX_SLOT_DW; q++) r.l[q] = src[vec * SIX_SLOT_DW + q];
}
extern "C" __global__ void __launch_bounds__(64, 2) H2V_NO_TAIL_MARK
k_probe_six(int op, uint32_t n, int csqr_n, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, const uint32_t *__restrict__ pts,
            const uint32_t *__restrict__ flags_in, const uint32_t *__restrict__ lines16, uint32_t *__restrict__ out, uint32_t *__restrict__ ok_out) {
    const int lane = threadIdx.x;
    Six c;
    const int grp = six_lane_setup(c, lane);
    const bool is_leader = c.act && c.k == 0;
    const uint32_t i = blockIdx.x * SIX_GROUPS + grp;
    const bool live = i < n;
    const uint32_t ii = live ? i : n - 1;
    six_tables_to_lds(lane);
    const bool lines = op == SIX_PROBE_LINE1 || op == SIX_PROBE_LINE2, round = op == SIX_PROBE_PROD2 || op == SIX_PROBE_ROUND;
    SixF2 x;
    six_probe_vec(x.re, a, (size_t)ii * 12 + 2 * c.k);
    six_probe_vec(x.im, a, (size_t)ii * 12 + 2 * c.k + 1);
    if (lines && c.act && c.k < 4) {           // the T slots, two per lane
        F28 t;
        six_probe_vec(t, b, (size_t)ii * 12 + 2 * c.k);
        six_store(six_slot(c, SIX_SLOT_T + 2 * c.k), t);
        six_probe_vec(t, b, (size_t)ii * 12 + 2 * c.k + 1);
        six_store(six_slot(c, SIX_SLOT_T + 2 * c.k + 1), t);
    }
    if (round && is_leader) {
        static_assert(SIX_SLOT_PY1 == SIX_SLOT_PX1 + 1 && SIX_SLOT_PX2 == SIX_SLOT_PX1 + 2 && SIX_SLOT_PY2 == SIX_SLOT_PX1 + 3, "the point slots are one run");
        for (int q = 0; q < 4; q++) {
            F28 t;
            six_probe_vec(t, pts, (size_t)ii * 4 + q);
            six_store(six_slot(c, SIX_SLOT_PX1 + q), t);
        }
    }
    const uint32_t flags = (lines || op == SIX_PROBE_ROUND) ? flags_in[ii] : 0u;
    const bool skip1 = (flags & 1) != 0, skip2 = (flags & 2) != 0;
    const int xs1 = SIX_PROD2_XS1(c.k), ys1 = SIX_PROD2_YS1(c.k);
    __syncthreads();

    SixF2 r = x;
    bool ok = true;
    switch (op) {
    case SIX_PROBE_MUL: {
        SixF2 y;
        six_probe_vec(y.re, b, (size_t)ii * 12 + 2 * c.k);
        six_probe_vec(y.im, b, (size_t)ii * 12 + 2 * c.k + 1);
        r = six_mul(c, x, y);
    } break;
    case SIX_PROBE_SQR: r = six_sqr(c, x); break;
    case SIX_PROBE_LINE1: r = six_line<1>(c, x, skip1); break;
    case SIX_PROBE_LINE2: r = six_line<2>(c, x, skip2); break;
    case SIX_PROBE_PROD2:
    case SIX_PROBE_ROUND: {
        if (op == SIX_PROBE_ROUND) r = six_sqr(c, x);
        six_line_store(six_line_share(lines16, 0, lane), lane);
        __syncthreads();
        six_prod2(c, xs1, ys1);
        if (op == SIX_PROBE_ROUND) {
            r = six_line<1>(c, r, skip1);
            r = six_line<2>(c, r, skip2);
        } else {
            __syncthreads();
            six_load_pair(r.re.l, r.im.l, six_slot(c, SIX_SLOT_T + c.k), six_slot(c, SIX_SLOT_T + 6 + (c.k & 1)));
        }
    } break;
    case SIX_PROBE_CSQR: r = six_csqr(c, x, csqr_n); break;
    case SIX_PROBE_CONJ: r = six_conj(c, x); break;
    case SIX_PROBE_FROB: r = six_frob(c, x); break;
    case SIX_PROBE_INV: {
        SixRegs fr;
        fr.re = f28_pack(x.re);
        fr.im = f28_pack(x.im);
        r = six_unpack(six_inv_raw(c, fr, ok));
    } break;
    case SIX_PROBE_FOLD:
        f28_fold(r.re);
        f28_fold(r.im);
        break;
    default: break;
    }
    if (!live || !c.act) return;
    if (op == SIX_PROBE_PROD2) {               // r: (T slot k, T slot 6 + (k & 1))
#pragma unroll
        for (int q = 0; q < SIX_SLOT_DW; q++) out[(size_t)i * SIX_PROBE_OUT_DW + c.k * SIX_SLOT_DW + q] = r.re.l[q];
        if (c.k < 2)
#pragma unroll
            for (int q = 0; q < SIX_SLOT_DW; q++) out[(size_t)i * SIX_PROBE_OUT_DW + (6 + c.k) * SIX_SLOT_DW + q] = r.im.l[q];
        return;
    }
#pragma unroll
    for (int q = 0; q < SIX_SLOT_DW; q++) {
        out[((size_t)i * 6 + c.k) * 2 * SIX_SLOT_DW + q] = r.re.l[q];
        out[((size_t)i * 6 + c.k) * 2 * SIX_SLOT_DW + SIX_SLOT_DW + q] = r.im.l[q];
    }
    if (op == SIX_PROBE_INV && c.k == 0) ok_out[i] = ok ? 1u : 0u;
}
