// C-ABI of the MI355X Halo2/KZG batch verifier (include/h2v.h).  Host side: plan parsing/validation/upload,
// workspace management, stream orchestration of the four kernels.  No arithmetic happens on the host and there
// is no CPU fallback: a missing or failing device is an error (H2V_E_DEVICE), never a silent detour.
#include "../../include/h2v.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "h2v_kernels.hip"
#include "h2v_mixed.hpp"
#include "h2v_mixed_dev.hpp"
#include "h2v_mixed_fold.hpp"
#include "h2v_mixed_fold_dev.hpp"
#include "h2v_mixed_srs.hpp"
#include "h2v_mixed_srs_dev.hpp"
#define H2V_GROUP_HD __host__ __device__ inline
#include "h2v_mixed_group.hpp"
#include "h2v_mixed_group_dev.hpp"
#include "h2v_aggregate_dev.hpp"
#include "h2v_msm_shape.hpp"
#include "h2v_pairing_engine.hpp"
#include "h2v_hostcall_layout.hpp"
#include "h2v_seed.hpp"
#include "h2v_mixed_tables.hpp"
#include "h2v_plancc.hpp"
#include "h2v_planblob.hpp"
#include "h2v_ws_layout.hpp"
using wslayout::vm_lds_slots;
using wslayout::msm_sum_width;
static_assert(sizeof(PipArgs) == PIP_ARGS_BYTES, "h2v_pip_sizes.hpp: the argument record of a bucket MSM");

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) {
    g_err = msg;
    if (code == H2V_E_DEVICE && msg.find("hip: ") == std::string::npos) {      // what the runtime said last on this thread, if anything
        const hipError_t e = hipPeekAtLastError();
        if (e != hipSuccess) g_err += std::string(" [hip: ") + hipGetErrorString(e) + "]";
    }
    return code;
}
#define HIPCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return fail(H2V_E_DEVICE, std::string(#expr) + ": hip: " + hipGetErrorString(e_));                \
    } while (0)

extern "C" const char *h2v_last_error(void) { return g_err.c_str(); }

// THE owner of device memory, pinned host memory and events.  Every block and every event of this file belongs to exactly one
// Owner - a member of the struct whose typed pointer fields name them (h2v_plan, h2v_workspace, HostSlot, Coalesce, PipWs, RlcWs,
// RlcWs::Grp, MixedWs, MixedWs::Slot) - which records WHERE the handle is kept, so that release() frees whatever was recorded and
// leaves every field NULL: a buffer added to a struct cannot be forgotten in a list, and a second release does nothing.  Each block
// is an allocation of its own (hipFree's implicit device wait and the alignment of every buffer depend on it).  No destructor:
// the holder releases after ITS waits, on the right device (ws_release, plan_release).  A holder must not move while its owner
// holds anything; assigning a fresh holder over a released one (`g = Grp()`) is the one copy there is, and both owners are empty.
// g_mem_live: what is live per device, for h2v_probe_device_memory - device blocks, device bytes, pinned blocks, pinned bytes, events.
static std::atomic<uint64_t> g_mem_live[16][5];
struct Owner {
    using Fill = wslayout::Fill;
    static constexpr Fill NONE = wslayout::NONE, ZERO = wslayout::ZERO, ONES = wslayout::ONES;
    struct Block { void **at; size_t bytes; bool pinned; };
    std::vector<Block> blocks;
    std::vector<hipEvent_t *> events;
    int dev = -1;                      // where everything recorded lives: the device that was current at the first allocation
    Owner() = default;
    Owner(const Owner &) = delete;
    Owner &operator=(const Owner &o) { if (!empty() || !o.empty()) abort(); return *this; }
    bool empty() const { return blocks.empty() && events.empty(); }
    void count(int what, uint64_t by) { if (dev >= 0 && dev < 16) g_mem_live[dev][what] += by; }
    bool take(void **at, size_t bytes, bool pinned, Fill fill) {
        *at = nullptr;
        if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = -1;
        if ((pinned ? hipHostMalloc(at, bytes, hipHostMallocDefault) : hipMalloc(at, bytes)) != hipSuccess) { *at = nullptr; return false; }
        if (!*at) return true;         // (a request of no bytes)
        blocks.push_back({at, bytes, pinned});
        count(pinned ? 2 : 0, 1); count(pinned ? 3 : 1, bytes);
        if (fill != NONE && pinned) memset(*at, fill, bytes);
        return fill == NONE || pinned || hipMemset(*at, fill, bytes) == hipSuccess;
    }
    template <class T> bool alloc(T *&field, size_t bytes, Fill fill = NONE) { return take((void **)&field, bytes, false, fill); }
    template <class T> bool alloc_pinned(T *&field, size_t bytes, Fill fill = NONE) { return take((void **)&field, bytes, true, fill); }
    // a row of a size table (h2v_ws_layout.hpp); a row of no bytes is a buffer the shape does not have
    template <class T> bool alloc(T *&field, const wslayout::Row &r) { return r.bytes == 0 || alloc(field, r.bytes, r.fill); }
    template <class T> bool alloc_pinned(T *&field, const wslayout::Row &r) { return r.bytes == 0 || alloc_pinned(field, r.bytes, r.fill); }
    bool event(hipEvent_t &e, unsigned flags) {
        if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = -1;
        if (hipEventCreateWithFlags(&e, flags) != hipSuccess) { e = nullptr; return false; }
        events.push_back(&e);
        count(4, 1);
        return true;
    }
    void free_block(const Block &b) {
        if (*b.at) (void)(b.pinned ? hipHostFree(*b.at) : hipFree(*b.at));
        *b.at = nullptr;
        count(b.pinned ? 2 : 0, (uint64_t)0 - 1); count(b.pinned ? 3 : 1, (uint64_t)0 - b.bytes);
    }
    // one block back, the rest stays (a block that is re-allocated larger); a field this owner does not hold is left alone
    template <class T> void drop(T *&field) {
        for (size_t k = 0; k < blocks.size(); k++)
            if (blocks[k].at == (void **)&field) { free_block(blocks[k]); blocks.erase(blocks.begin() + (long)k); return; }
    }
    void release() {
        for (const Block &b : blocks) free_block(b);
        for (hipEvent_t *e : events) { (void)hipEventDestroy(*e); *e = nullptr; count(4, (uint64_t)0 - 1); }
        blocks.clear(); events.clear();
    }
};
// A block of device (PINNED = false) or pinned host memory that grows on demand, and THE slack rule of every staging block of this
// file: a request that does not fit frees the block and allocates a quarter more than was asked for, so that a caller whose
// batches creep upwards does not re-allocate at every call.  What may still be using the old block differs from site to site:
// the caller passes its wait as `quiet`, which runs before the free (its error is returned and the block stays).  The block
// belongs to the holder's Owner `mem`, which frees it with the holder's other blocks.
template <bool PINNED> struct GrowBuf {
    uint8_t *p = nullptr;
    size_t cap = 0;
    template <class Quiet> int ensure(Owner &mem, size_t need, const char *what, Quiet &&quiet) {
        if (need <= cap) return H2V_OK;
        if (int rc = quiet()) return rc;
        mem.drop(p);
        cap = 0;
        const size_t c = wslayout::grown(need);
        if (!(PINNED ? mem.alloc_pinned(p, c) : mem.alloc(p, c))) return fail(H2V_E_DEVICE, std::string("allocation of ") + what + " failed");
        cap = c;
        return H2V_OK;
    }
};
// an event created when first needed (one that exists stays)
static int lazy_event(Owner &mem, hipEvent_t &e, unsigned flags) {
    if (e || mem.event(e, flags)) return H2V_OK;
    return fail(H2V_E_DEVICE, std::string("hipEventCreate: hip: ") + hipGetErrorString(hipPeekAtLastError()));
}
static int no_wait() { return H2V_OK; }      // (a GrowBuf whose old block nothing can still be using)

// ---------------------------------------------------------------------------------------------- lifecycle
// Everything the library owns on a device - the pool of CU-mask streams (make_stream), every live workspace's buffers,
// streams and events, every plan's device memory - is released by h2v_shutdown(device), which a host calls before the
// process exits (backend.py: atexit; h2v.hpp: h2v::shutdown; the library itself registers it with atexit() when the first
// pool stream is created, i.e. after the HIP runtime's own initialisation, so that it runs BEFORE the runtime's exit
// handlers).  Why: a stream with a hardware queue of its own that is still alive when the runtime and a profiler's tool
// library run their static destructors was the exit-time SIGSEGV of round 3 (under rocprofv3, after "tool
// finalization", through __cxa_finalize: only the forms that had created pool streams crashed).  After the call every
// entry point that needs the device returns H2V_E_DEVICE; handles stay valid as empty shells and are freed as usual.
static std::mutex g_reg_mu;
static std::vector<h2v_workspace *> g_ws_live;
static std::vector<h2v_plan *> g_plan_live;
static bool g_shut[16] = {};
static bool dev_shut(int dev) {
    std::lock_guard<std::mutex> lock(g_reg_mu);
    return dev >= 0 && dev < 16 && g_shut[dev];
}
#define ALIVE_DEV(dev)                                                                                   \
    do {                                                                                                 \
        if (dev_shut(dev)) return fail(H2V_E_DEVICE, "h2v_shutdown has been called for this device");    \
    } while (0)
#define ALIVE(obj)                                                                                       \
    do {                                                                                                 \
        if ((obj) && (obj)->dead) return fail(H2V_E_DEVICE, "h2v_shutdown has been called: this handle is an empty shell"); \
    } while (0)
template <class T> static void reg_add(std::vector<T *> &v, T *x) { std::lock_guard<std::mutex> lock(g_reg_mu); v.push_back(x); }
template <class T> static void reg_del(std::vector<T *> &v, T *x) {
    std::lock_guard<std::mutex> lock(g_reg_mu);
    for (size_t i = 0; i < v.size(); i++) if (v[i] == x) { v[i] = v.back(); v.pop_back(); return; }
}
// content hash of csrc/ + include/h2v.h this binary was built from (__graft_entry__.build_hip compares it with the tree)
#ifndef H2V_SRC_HASH_STR
#define H2V_SRC_HASH_STR "unknown"
#endif
extern "C" const char *h2v_build_id(void) {
    static const char id[] = "H2V_SRC_HASH=" H2V_SRC_HASH_STR;
    return id + 13;
}
extern "C" int h2v_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---------------------------------------------------------------------------------------------- plan compiler
// VerifyingKey description (JSON, docs/vk_schema.json) -> plan blob, on the host: no GPU is needed for this call.
extern "C" int h2v_plan_compile(const char *vk_json, size_t len, uint8_t **blob_out, size_t *blob_len) {
    if (!vk_json || !blob_out || !blob_len) return fail(H2V_E_ARG, "null argument");
    *blob_out = nullptr; *blob_len = 0;
    try {
        const h2vplan::VK vk = h2vplan::parse_vk(vk_json, len);
        const std::vector<uint8_t> blob = h2vplan::compile_plan(vk);
        uint8_t *out = (uint8_t *)malloc(blob.size());
        if (!out) return fail(H2V_E_DEVICE, "out of memory");
        memcpy(out, blob.data(), blob.size());
        *blob_out = out; *blob_len = blob.size();
        return H2V_OK;
    } catch (const h2vplan::CompileError &e) {
        return fail(H2V_E_ARG, std::string("verifying-key description: ") + e.what());
    } catch (const std::exception &e) {
        return fail(H2V_E_ARG, std::string("plan compiler: ") + e.what());
    }
}
extern "C" void h2v_blob_free(uint8_t *blob) { free(blob); }

struct h2v_plan {
    int device = 0;
    bool dead = false;         // h2v_shutdown released the device memory: every call with this plan is H2V_E_DEVICE
    H2vDevPlan d{};            // device view
    Owner mem;                 // of the five blocks below
    void *blob = nullptr;      // one device allocation holding every section
    void *fold_terms = nullptr;  // recursion: the 4-entry term table of the two fold MSMs
    void *vk_tab = nullptr;      // window tables of the VK bases (k_vk_tables at load)
    void *fix_tab = nullptr;     // all-window tables of the VK bases (k_vk_fixed_tables at load; non-recursive plans)
    void *six_tab = nullptr;     // unit-coefficient line constants of the six-lane pairing engine + its dump constants (six_line_tables)
    uint32_t n_var = 0, n_fix = 0;  // per-proof terms [0, n_var), VK-base terms [n_var, n_var + n_fix) when the list is so ordered
    uint32_t n_squeezes = 0, stream_len = 0;
    uint32_t tr_kind = 0, tr_key_len = 0;   // transcript hash of the key (H2V_TRANSCRIPT_*) and its blake2b key
    uint8_t tr_key[H2V_TR_KEY_MAX] = {};
    uint64_t gen = 0;            // process-wide load counter: what caches key on (a freed plan's address may be reused)
    uint64_t sg2_digest[2] = {}; // of the s_g2 line-table section of the blob: plans of ONE SRS agree in it (h2v_verify_mixed)
    uint8_t key_tag[32] = {};    // blake2b-256(TAG key || the plan blob): what a derived batch seed binds the key with (h2v_seed.hpp)
    std::vector<uint32_t> trace_slots;
};

struct h2v_workspace {
    int device = 0;
    bool dead = false;             // h2v_shutdown released everything: an empty shell until h2v_workspace_free
    uint32_t in_flight_hint = 1;   // h2v_workspace_hint_in_flight: how many batches the caller keeps in flight on this device
    bool hint_given = false;       // (laned: the caller said so itself; otherwise run_laned estimates it per call)
    uint64_t cap = 0;       // max batch
    uint32_t stride = 0;    // register-file stride (cap rounded up to 64)
    Owner mem;              // of every block and event named by a field of this struct itself (HostSlot, lanes and the lazy sets own theirs)
    // what the buffers were sized for (the creating plan's shape, or the union of several): a plan fits iff wslayout::fits says so.
    // A laned workspace: the shape its lanes are created with when first used
    wslayout::Shape shape;
    uint32_t *regs = nullptr, *scalars = nullptr, *pts = nullptr, *er = nullptr, *status = nullptr, *trace = nullptr, *msm_tab = nullptr;
    // recursion (IVC): acc_left / acc_right_final sums, the fold's points + scalars, and the folded el / er
    uint32_t *accl = nullptr, *accr = nullptr, *fold_pts = nullptr, *fold_scal = nullptr, *el2 = nullptr, *er2 = nullptr;
    uint32_t *pt_tab = nullptr;  // MSM window tables of every per-proof point, written by the decompression kernel
    uint32_t *er_fix = nullptr;  // sum of the VK-base terms when the MSM is split into a ladder and a fixed-base launch
    // partial sums of a segmented MSM, [segment][proof][36 dwords] (plans with a sum of more than 64 terms only): room for
    // shape.segs segments of cap proofs (msm_max_segments of the widest sum the workspace was created for)
    uint32_t *msm_parts = nullptr;
    uint32_t *dec_ctr = nullptr; // work-queue counter of the decompression launch
    uint8_t *valid = nullptr, *valid_sub = nullptr, *accept = nullptr;
    // pair check (run_check): the two-slot view of 96-byte records - offsets 96 i (cap + 1 entries) and the slot table {0, 48} -
    // allocated and filled by the first check call on this workspace
    uint64_t *pair_off = nullptr;
    uint32_t *pair_pts = nullptr;
    // THE result block of the blocking host-buffer forms (prepare, pair check, aggregate, mixed): the device memory their kernels
    // write and the downloads read, laid out per call by hostcall::result_block.  One block serves every form because each of
    // them synchronises `hs` before it returns (host_call_tail) or drains every stream on error: no two calls ever use it at once.
    GrowBuf<false> res;
    // Host-buffer entry points: the batch is packed into ONE pinned host block (offsets | instances | committed | proofs),
    // uploaded with one asynchronous copy on the workspace's own stream `hs`, verified there, and the accept bytes come
    // back into pinned memory the same way: h2v_verify_batch_submit returns once everything is enqueued, _wait collects.
    // An ordinary workspace stages its one batch in hslot[0] (below); accept[] comes back from `accept`.
    hipStream_t hs = nullptr;
    bool pending = false;
    // the streams of the pipeline (ws_streams): the transcript + combiner kernel and everything after it on pmain, the
    // decompression beside it on pside
    hipStream_t pmain = nullptr, pside = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_hold = nullptr, ev_fix = nullptr, ev_done = nullptr;
    // ONE record per call of any kind, in a ring: call number k (absolute, counted from 0) is rec[k % RING] until call k + RING
    // takes the slot, so a lookup compares the record's own number with the one it wants (rec_at)
    static constexpr int RING = 64, NEV = 12, MAXL = 16;
    enum Kind : uint8_t { VERIFY, PREPARE, CHECK, RLC };
    struct CallRec {
        uint64_t call = ~0ull;
        Kind kind = VERIFY;
        bool no_vm = false;        // an RLC call over pairs from anywhere: no transcript ran (transcript_combiner_ms = 0)
        bool routed = false;       // an RLC call sent straight to the per-proof kernels (rlc_route): per-proof times, no batch check
        bool agg = false;          // an aggregate call (h2v_aggregate_batch / _mixed): the sums were exported, no pairing ran ("not checked")
        bool derived = false;      // its seed was derived from the batch (H2V_RLC_SEED_TRANSCRIPT): seed_ring holds it
        bool co = false, ran = false;   // coalesced (coalesce_call); its group has run - only then is the rest filled in (co_flush_lane)
        float share = 0.0f;        // coalesced: its proofs / the group's
        // ordinary workspace: the event set, created with the workspace.  Per proof (run_pipeline; run_check a subset):
        // [0]/[1] around the transcript+combiner kernel, [2]/[3] around the decompression kernel (side stream), [4]/[5] around
        // the MSM, [5]/[6] around the pairing kernel, [7]/[8] around the fixed-base MSM launch of a split MSM, [9] the end of the
        // ladder launch beside it, [10]/[11] mark the MSM's hold and are not read.  RLC: run_rlc's eleven.
        hipEvent_t ev[NEV] = {};
        uint8_t lpt = 0, var_lpt = 0, pair = 0;   // MSM lanes per term (3: split), the ladder half of a split MSM, pairing lanes (0: none ran)
        uint32_t rlc_terms = 0, rlc_c = 0, rlc_W = 0, rlc_chain = 0;   // RLC: the bucket MSM's terms, window bits, windows, chain
        // laned workspace: chunk c ran on lane (first + c) % mod as that lane's record start[lane] + c / mod (a coalesced call:
        // one "chunk", its group's run)
        uint32_t first = 0, mod = 1, chunks = 0;
        uint64_t start[MAXL] = {};
    };
    CallRec rec[RING];
    uint64_t calls = 0;
    uint32_t *rec_fail = nullptr;   // RING device words: failed batch checks of record k at [k % RING] (RLC calls; rlc_stats_ensure)
    // derived seeds (H2V_RLC_SEED_TRANSCRIPT; seed_enqueue): RING slots of 8 device dwords, the seed of record k at [k % RING] as
    // rec_fail is indexed - it outlives the call's kernels; the digest buffer of the call being derived (h2v_seed.hpp: Tree), which
    // the next derivation reuses behind ev_seed[..][1] of this one; per slot the two timed events around the digest launches
    uint32_t *seed_ring = nullptr;
    GrowBuf<false> seed_digests;
    hipEvent_t ev_seed[RING][2] = {};
    hipEvent_t ev_seed_last = nullptr;      // the end of the most recent derivation (one of ev_seed[..][1])
    struct RlcWs *rlc = nullptr;   // buffers of the RLC batch mode, created by its first call
    struct RlcWs *prlc = nullptr;  // the pair-RLC set (h2v_check_pairs_rlc, H2V_RLC_FOLD_PAIRS): created by the first such call
    struct MultiWs *multi = nullptr;   // the set of h2v_check_pairs_multi (several SRS in one check): created by the first such call
    hipEvent_t ev_pipe[12] = {};   // H2V_RLC_FOLD_PAIRS: the pipeline's own markers (the record's events carry the RLC layout)
    std::vector<struct RlcWs *> rlc_parked;   // the same for OTHER plans this workspace has served in that mode (rlc_ensure swaps; never freed before the workspace)
    int32_t opt[H2V_OPT_COUNT] = {};   // h2v_workspace_set_option / h2v_workspace_tune: 0 = the launcher's choice
    int one_stream_mode = -1;      // lanes: 1 = the whole pipeline on the stream it is given (-1: decided from the hint)
    // ---- lanes (h2v_workspace_create_lanes): a laned workspace owns no kernel buffers of its own, only n_lanes ordinary
    // workspaces of `chunk` proofs and one library-owned stream per lane.  A verify call is cut into chunks that go round
    // robin through the lanes; chunk c of a call runs entirely on lane_st[lane of c], behind that lane's earlier chunks.
    uint32_t n_lanes = 0, chunk = 0;
    h2v_workspace *lane[MAXL] = {};
    hipStream_t lane_st[MAXL] = {};
    hipEvent_t lane_ev[MAXL] = {};         // end of the lane's most recent chunk
    bool lane_busy[MAXL] = {};             // work enqueued since the last join
    bool defer_joins = false;
    uint32_t lanes_per_proof = 0;           // lanes the per-proof mode cycles through (the RLC mode uses all n_lanes)
    uint64_t next_lane = 0;                 // round-robin position (persists across calls: consecutive calls interleave)
    // host-buffer batches in flight on a laned workspace (h2v_verify_batch_submit / _wait): a ring of staging slots, each
    // with its own pinned block, device block and accept buffers; uploads on `hs`, downloads on `hs_down` (stage_batch)
    struct HostSlot {
        Owner mem;
        GrowBuf<false> in_block, d_accept;      // (d_accept: laned only)
        GrowBuf<true> h_block, h_accept;
        hipEvent_t ev = nullptr;
        uint64_t n = 0;
        bool rlc = false;
    };
    static constexpr int MAXH = 16;
    HostSlot hslot[MAXH];
    uint64_t h_head = 0, h_tail = 0;
    hipStream_t hs_down = nullptr;
    bool copy_streams_owned = false;        // laned: hs / hs_down carry copies only and are plain streams of this workspace (host_stream)
    // routing of RLC calls by what earlier calls met (rlc_route): cumulative device counters [groups seen, groups failed], a
    // pinned host mirror refreshed behind every call, and the running estimate of the failing-group rate
    uint32_t *rlc_stats = nullptr, *rlc_stats_ptr = nullptr, *h_rlc_stats = nullptr;
    uint32_t seen_groups = 0, seen_failed = 0;
    float fail_rate = 0.0f;
    bool routed = false;                    // the most recent RLC call ran the per-proof kernels directly
    // ---- coalescing of small device-resident calls (coalesce_call): per lane a staging area the proofs of several calls are
    // gathered into; co_open: the lanes whose groups are open, oldest first (one group per plan and mode, at most four)
    struct Coalesce *co[MAXL] = {};
    struct MixedWs *mixed = nullptr;        // staging of the mixed-key calls (h2v_verify_mixed), created by the first one
    // aggregate calls (h2v_aggregate_batch / _mixed): the parts buffer, parts of [2][36] dwords - every chunk's two
    // Jacobian sums, which k_aggregate_export adds.  AGG_SLOTS fixed slots of AGG_SLOT_PARTS parts each, one per call in flight, so
    // that calls on several caller streams overlap; a call of more parts takes the whole buffer (agg_ensure has the invariant)
    static constexpr uint32_t AGG_SLOTS = 16, AGG_SLOT_PARTS = 128;     // (as many calls as a workspace has lanes)
    GrowBuf<false> agg_parts;
    uint64_t agg_calls = 0;
    hipEvent_t ev_agg[AGG_SLOTS] = {};
    bool agg_used[AGG_SLOTS] = {};
    std::vector<uint32_t> co_open;
};
using CallRec = h2v_workspace::CallRec;
// the record of the call being made on w (every call takes exactly one), and the record of call number `call` while no later
// call has taken its slot (NULL once one has)
static CallRec &rec_new(h2v_workspace *w, h2v_workspace::Kind kind) {
    CallRec &r = w->rec[w->calls % h2v_workspace::RING];
    CallRec fresh;
    memcpy(fresh.ev, r.ev, sizeof fresh.ev);   // (the event set belongs to the slot)
    r = fresh;
    r.call = w->calls++;
    r.kind = kind;
    return r;
}
static CallRec *rec_at(h2v_workspace *w, uint64_t call) {
    CallRec &r = w->rec[call % h2v_workspace::RING];
    return r.call == call ? &r : nullptr;
}
static CallRec &rec_last(h2v_workspace *w) { return w->rec[(w->calls - 1) % h2v_workspace::RING]; }
static uint32_t *rec_word(h2v_workspace *w, const CallRec &r) { return w->rec_fail + r.call % h2v_workspace::RING; }

// ---------------------------------------------------------------------------------------------- plan
static void plan_release(h2v_plan *p) {   // the device memory; the host-side facts (h2v_plan_info) stay
    (void)hipSetDevice(p->device);
    p->mem.release();
}
// All-window tables of the VK bases for the fixed-base launches of the MSM (planblob::fixed_tables has the shape): every window
// multiple of every VK base.  The window bases are a temporary block of this function.
static bool plan_fixed_tables(h2v_plan *p, const planblob::FixedTables &ft) {
    const uint32_t n_bases = p->d.n_vk_bases;
    Owner tmp;
    void *wbase = nullptr;
    bool ok = p->mem.alloc(p->fix_tab, ft.bytes + 16, Owner::ZERO) && tmp.alloc(wbase, (size_t)n_bases * ft.W * 96 + 16);
    if (ok) {
        hipLaunchKernelGGL(k_vk_fixed_window_bases, dim3((n_bases * ft.W + 63) / 64), dim3(64), 0, nullptr, p->d.vk_bases, n_bases, ft.c, ft.W, (uint32_t *)wbase);
        const uint64_t entries = (uint64_t)n_bases * ft.W * ft.entries;
        hipLaunchKernelGGL(k_vk_fixed_tables, dim3((uint32_t)((entries + 63) / 64)), dim3(64), 0, nullptr, (const uint32_t *)wbase, n_bases * ft.W, ft.c, (uint32_t *)p->fix_tab);
        ok = hipDeviceSynchronize() == hipSuccess;
    }
    tmp.release();
    return ok;
}
// What a load learns on the host: the device view of the uploaded blob (the table pointers follow as the tables are built)
// and the facts the plan's own entry points answer from (h2v_plan_transcript, _key_tag, _same_srs, _trace_slots).
static void plan_fill(h2v_plan *p, const planblob::View &v, const uint8_t *blob, size_t len) {
    auto at = [&](uint32_t off) { return (const uint32_t *)((const uint8_t *)p->blob + off); };
    H2vDevPlan &d = p->d;
    d.proof_len = v.proof_len; d.n_pi = v.n_pi; d.n_ci = v.n_ci; d.n_consts = v.n_consts;
    d.n_points = v.n_points; d.n_vk_bases = v.n_bases; d.n_terms = v.n_terms; d.n_trace = v.n_trace; d.pi_point = v.pi_point;
    d.instr = (const H2vInstr *)at(v.narrow.off);
    d.n_instr = v.narrow.n_instr; d.n_regs = v.narrow.n_regs; d.vm_lanes = v.narrow.lanes;
    if (v.wide.lanes) {
        d.wide_lanes = v.wide.lanes; d.wide_n_regs = v.wide.n_regs; d.wide_n_instr = v.wide.n_instr;
        d.wide_instr = (const H2vInstr *)at(v.wide.off);
    }
    d.consts = at(v.off_consts); d.points = at(v.off_points); d.vk_bases = at(v.off_bases); d.terms = at(v.off_terms); d.trace = at(v.off_trace);
    d.lines_sg2 = at(v.off_lines_sg2); d.lines_g2 = at(v.off_lines_g2); d.lines28_sg2 = at(v.off_lines28_sg2); d.lines28_g2 = at(v.off_lines28_g2);
    d.ivc = v.ivc; d.n_main_terms = v.n_main_terms;
    memcpy(d.acc_idx, v.acc_idx, sizeof d.acc_idx);
    d.fold_terms = (const uint32_t *)p->fold_terms;
    p->tr_kind = d.tr_kind = v.tr_kind;
    p->tr_key_len = v.tr_key_len;
    if (v.tr_key_len) memcpy(p->tr_key, blob + v.tr_key_off, v.tr_key_len);
    if (v.tr_kind == H2V_TR_BLAKE2B_512) d.tr_t0 = planblob::transcript_midstate(blob, v, d.tr_h0);
    planblob::sg2_digest(blob, v, p->sg2_digest);
    planblob::key_tag(blob, len, p->key_tag);
    p->n_squeezes = v.n_squeezes; p->stream_len = v.stream_len; p->trace_slots = v.trace_slots;
}
extern "C" int h2v_plan_load(const uint8_t *blob, size_t len, int device, h2v_plan **out) { return h2v_plan_load_ex(blob, len, device, nullptr, out); }
extern "C" int h2v_plan_load_ex(const uint8_t *blob, size_t len, int device, const h2v_plan_opts *opts, h2v_plan **out) {
    // 1. the arguments
    if (!blob || !out) return fail(H2V_E_ARG, "null argument");
    const uint32_t opt_fix_c = opts ? opts->fixed_base_window_bits : 0u;
    if (opt_fix_c != 0 && opt_fix_c != 4 && opt_fix_c != 8 && opt_fix_c != 12) return fail(H2V_E_ARG, "fixed_base_window_bits: 0 (auto), 4, 8 or 12");
    *out = nullptr;
    // 2. the blob, validated completely on the host before any device work (h2v_planblob.hpp)
    planblob::View v;
    std::string why;
    if (int rc = planblob::parse(blob, len, v, why)) return fail(rc, why);
    // 3. the device
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(H2V_E_DEVICE, "no HIP device: the HIP backend is required (no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(H2V_E_ARG, "device index out of range");
    ALIVE_DEV(device);
    HIPCHK(hipSetDevice(device));
    h2v_plan *p = new h2v_plan();
    p->device = device;
    // THE failure exit from here on: whatever has been allocated so far goes the way h2v_plan_free would send it
    auto give_up = [&](const char *what) { plan_release(p); delete p; return fail(H2V_E_DEVICE, what); };
    // 4. the blob on the device, its term table as the MSM kernel wants it (planblob::device_terms)
    if (!p->mem.alloc(p->blob, len)) return give_up("hipMalloc(plan) failed");
    if (v.ivc) {
        const uint32_t ft[8] = {H2V_TERM_PROOF_POINT, 0, H2V_TERM_PROOF_POINT, 1, H2V_TERM_PROOF_POINT, 2, H2V_TERM_PROOF_POINT, 3};
        if (!p->mem.alloc(p->fold_terms, sizeof ft) || hipMemcpy(p->fold_terms, ft, sizeof ft, hipMemcpyHostToDevice) != hipSuccess)
            return give_up("fold term upload failed");
    }
    {
        std::vector<uint8_t> patched(blob, blob + len);
        const std::vector<uint8_t> terms = planblob::device_terms(blob, v);
        memcpy(patched.data() + v.off_terms, terms.data(), terms.size());
        if (hipMemcpy(p->blob, patched.data(), len, hipMemcpyHostToDevice) != hipSuccess) return give_up("plan upload failed");
    }
    // 5. the device view and the host-side facts, from the View
    plan_fill(p, v, blob, len);
    H2vDevPlan &d = p->d;
    // 6. the tables.  Window tables of the VK bases for the MSM ladder: [1..8]B and [1..8]phi(B), affine, computed once per plan
    const size_t vk_tab_bytes = (size_t)v.n_bases * 448 * 4 + 16;
    if (!p->mem.alloc(p->vk_tab, vk_tab_bytes, Owner::ZERO)) return give_up("hipMalloc(vk tables) failed");
    if (v.n_bases) {
        hipLaunchKernelGGL(k_vk_tables, dim3((v.n_bases + 63) / 64), dim3(64), 0, nullptr, d.vk_bases, v.n_bases, (uint32_t *)p->vk_tab);
        if (hipDeviceSynchronize() != hipSuccess) return give_up("VK window-table kernel failed");
    }
    d.vk_tab = (const uint32_t *)p->vk_tab;
    std::vector<uint32_t> six;   // the six-lane pairing engine's own line constants (host math, once per plan)
    if (planblob::six_line_tables(blob, v, six)) {
        if (!p->mem.alloc(p->six_tab, six.size() * 4) || hipMemcpy(p->six_tab, six.data(), six.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            return give_up("six-lane line table upload failed");
        d.six_norm28 = (const uint32_t *)p->six_tab;
        d.six_k = d.six_norm28 + planblob::SIX_NORM_DW;
    }
    if (v.n_fix) {   // the fixed-base launches of the MSM (tests force the window width: h2v_plan_opts)
        const planblob::FixedTables ft = planblob::fixed_tables(v.n_bases, opt_fix_c);
        if (!plan_fixed_tables(p, ft)) return give_up("fixed-base table setup failed");
        d.fix_c = ft.c; d.fix_W = ft.W;
        p->n_var = v.n_var; p->n_fix = v.n_fix;
    }
    d.fix_tab = (const uint32_t *)p->fix_tab; d.n_var = p->n_var; d.n_fix = p->n_fix;
    // 7. the registry
    { static std::mutex mu; static uint64_t loads = 0; std::lock_guard<std::mutex> lock(mu); p->gen = ++loads; }
    reg_add(g_plan_live, p);
    *out = p;
    return H2V_OK;
}
extern "C" void h2v_plan_free(h2v_plan *p) {
    if (!p) return;
    reg_del(g_plan_live, p);
    if (!p->dead) plan_release(p);
    delete p;
}
extern "C" int h2v_plan_info(const h2v_plan *p, uint32_t *proof_len, uint32_t *n_pi, uint32_t *n_ci, uint32_t *n_terms) {
    if (!p) return fail(H2V_E_ARG, "null plan");
    if (proof_len) *proof_len = p->d.proof_len;
    if (n_pi) *n_pi = p->d.n_pi;
    if (n_ci) *n_ci = p->d.n_ci;
    if (n_terms) *n_terms = p->d.n_terms;
    return H2V_OK;
}
extern "C" int h2v_plan_transcript(const h2v_plan *p, uint32_t *kind, uint8_t key_out[64], uint32_t *key_len) {
    if (!p) return fail(H2V_E_ARG, "null plan");
    if (kind) *kind = p->tr_kind;
    if (key_out) { memset(key_out, 0, H2V_TR_KEY_MAX); memcpy(key_out, p->tr_key, p->tr_key_len); }
    if (key_len) *key_len = p->tr_key_len;
    return H2V_OK;
}
extern "C" int h2v_plan_key_tag(const h2v_plan *p, uint8_t out[32]) {
    if (!p || !out) return fail(H2V_E_ARG, "null argument");
    memcpy(out, p->key_tag, 32);
    return H2V_OK;
}
extern "C" int h2v_plan_same_srs(const h2v_plan *a, const h2v_plan *b) {
    if (!a || !b) return fail(H2V_E_ARG, "null argument");
    return memcmp(a->sg2_digest, b->sg2_digest, sizeof a->sg2_digest) == 0 ? 1 : 0;
}
extern "C" int h2v_plan_trace_slots(const h2v_plan *p, uint32_t *slot_ids, uint32_t cap, uint32_t *n_out) {
    if (!p || !n_out) return fail(H2V_E_ARG, "null argument");
    *n_out = (uint32_t)p->trace_slots.size();
    for (uint32_t k = 0; k < cap && k < p->trace_slots.size(); k++) slot_ids[k] = p->trace_slots[k];
    return H2V_OK;
}

// ---------------------------------------------------------------------------------------------- workspace
static void rlc_release(struct RlcWs *r);
static hipError_t make_stream(hipStream_t *s);
static void co_release(h2v_workspace *w);
static void mixed_release(h2v_workspace *w);
static void multi_release(h2v_workspace *w);
static int co_flush(h2v_workspace *w);
static int lane_streams(uint32_t l, hipStream_t *main_st, hipStream_t *side_st);
static void slot_release(h2v_workspace::HostSlot &sl) {
    sl.mem.release();
    sl = h2v_workspace::HostSlot();
}
static void ws_release(h2v_workspace *w) {
    (void)hipSetDevice(w->device);
    // the waits, all of them before anything is freed: the copy streams, the lanes' streams, the pipeline's (pool streams are
    // shared: make_stream; h2v_shutdown destroys them); mixed_release and every lane's own ws_release wait for what is theirs
    for (hipStream_t q : {w->hs_down, w->hs, w->pmain, w->pside}) if (q) (void)hipStreamSynchronize(q);
    for (hipStream_t q : w->lane_st) if (q) (void)hipStreamSynchronize(q);
    // then one release per owner
    mixed_release(w);
    for (h2v_workspace *&lw : w->lane)
        if (lw) { ws_release(lw); delete lw; lw = nullptr; }
    w->n_lanes = 0;
    for (auto &sl : w->hslot) slot_release(sl);
    co_release(w);                        // (an open group is dropped: whoever frees a workspace has joined it or no longer wants the verdicts)
    if (w->rlc) { rlc_release(w->rlc); w->rlc = nullptr; }
    for (struct RlcWs *r : w->rlc_parked) rlc_release(r);
    w->rlc_parked.clear();
    if (w->prlc) { rlc_release(w->prlc); w->prlc = nullptr; }
    multi_release(w);
    w->mem.release();
    w->ev_seed_last = nullptr;
    if (w->copy_streams_owned) {
        if (w->hs) (void)hipStreamDestroy(w->hs);
        if (w->hs_down) (void)hipStreamDestroy(w->hs_down);
        w->hs = w->hs_down = nullptr; w->copy_streams_owned = false;
    }
}
// An ordinary workspace (or a lane) of max_batch proofs for plans that fit shape s: the rows of wslayout::pipeline, in their order
static int ws_create_for(const wslayout::Shape &s, int device, uint64_t max_batch, h2v_workspace **out) {
    if (max_batch == 0 || max_batch > (1ull << 24)) return fail(H2V_E_ARG, "max_batch out of range");
    ALIVE_DEV(device);
    HIPCHK(hipSetDevice(device));
    h2v_workspace *w = new h2v_workspace();
    w->device = device;
    w->cap = max_batch;
    w->stride = (uint32_t)((max_batch + 63) / 64 * 64);
    w->shape = s;
    const auto T = wslayout::pipeline(s, max_batch);
    const wslayout::Row *failed = nullptr;
    auto row = [&](auto *&field, wslayout::Pipe k) { if (!failed && !w->mem.alloc(field, T.row[k])) failed = &T.row[k]; };
    row(w->regs, wslayout::P_REGS); row(w->scalars, wslayout::P_SCALARS); row(w->pts, wslayout::P_PTS); row(w->valid, wslayout::P_VALID);
    row(w->valid_sub, wslayout::P_VALID_SUB); row(w->dec_ctr, wslayout::P_DEC_CTR); row(w->er_fix, wslayout::P_ER_FIX);
    row(w->msm_parts, wslayout::P_MSM_PARTS); row(w->er, wslayout::P_ER); row(w->pt_tab, wslayout::P_PT_TAB); row(w->msm_tab, wslayout::P_MSM_TAB);
    row(w->status, wslayout::P_STATUS); row(w->accept, wslayout::P_ACCEPT); row(w->trace, wslayout::P_TRACE); row(w->accl, wslayout::P_ACCL);
    row(w->accr, wslayout::P_ACCR); row(w->el2, wslayout::P_EL2); row(w->er2, wslayout::P_ER2); row(w->fold_pts, wslayout::P_FOLD_PTS);
    row(w->fold_scal, wslayout::P_FOLD_SCAL);
    if (failed) { const std::string what = failed->name; ws_release(w); delete w; return fail(H2V_E_DEVICE, "hipMalloc(" + what + ") failed"); }
    // Streams are created on first use (ws_streams): the runtime maps streams onto a few hardware queues round robin, and
    // streams that are never used would only make the ones in use collide (several batches in flight: bench.py --inflight).
    bool ok = true;
    for (hipEvent_t *e : {&w->ev_fork, &w->ev_join, &w->ev_hold, &w->ev_fix, &w->ev_done})
        if (ok) ok = w->mem.event(*e, hipEventDisableTiming);
    for (CallRec &r : w->rec) for (hipEvent_t &e : r.ev)
        if (ok) ok = w->mem.event(e, hipEventDefault);
    if (!ok) { ws_release(w); delete w; return fail(H2V_E_DEVICE, "stream/event creation failed"); }
    *out = w;
    return H2V_OK;
}
// Chunk size of the lanes: the batch that gives the kernels of the per-proof pipeline about one wave per SIMD - the merged
// MSM runs one lane per (proof, term): 65536 / T proofs for 1024 waves (T = 16: 4096, the BASELINE batch; T = 60: 1092) -
// as a power of two between 1024 and 4096.
static uint32_t default_chunk(const wslayout::Shape &s) {
    const double want = 65536.0 / (double)(s.main_terms ? s.main_terms : 1);
    uint32_t c = 1024;
    while (c < 4096 && (double)c * 1.4142 < want) c <<= 1;
    return c;
}
// What a LANE holds (h2v_workspace_create_lanes with chunk = 0): 4096 proofs whatever the plan.  With several batches in flight
// the launch that pays is the large one - the six-lane pairing engine, ladders that share their doublings, fewer and longer
// launches - and since small calls are gathered (coalesce_call) a lane's capacity is no longer the size of the calls.  Measured,
// ms per call of the BASELINE size with the lanes at default_chunk -> 4096 (-> 8192): lookup_table x 2048 3.17 -> 2.92 (2.86),
// atms x 2048 3.30 -> 2.78 (2.70), sha256 shape x 1024 1.96 -> 1.86 (1.87), secp256k1 x 512 1.01 -> 0.87, their shares x 128 / x 64
// 0.32 / 0.17 -> 0.27 / 0.15; simple_mul x 4096 is at 4096 already (8192: the same).  A call that waits for its own chunks is
// still cut down to default_chunk / 2 per lane (run_laned).
static uint32_t lane_chunk() { return 4096u; }
// Lanes: measured on MI355X, simple_mul, a stream of 4096-proof batches through one laned workspace (deferred joins; ms per
// batch): per-proof mode, each lane's pipeline on the lane's stream with the decompression beside it on a side stream:
// 4 lanes 4.60, 5: 4.35, 6: 4.31, 11: 4.72; everything on the lane's stream: 5: 4.64, 8: 4.26, 11: 4.43 (five caller-owned
// workspaces on fifteen streams, round 2's bench: 4.50); RLC mode (one stream per lane): 8 lanes 1.65, 11: 1.54, 16: 1.47.
// With the split MSM, the 12-bit fixed-base tables and the six-lane pairing engine the per-proof optimum moved to 8 lanes
// (= the whole pool of 16 streams; 9 lanes share streams: 4.27): simple_mul x 4096 6: 3.88, 7: 3.86, 8: 3.76; atms x 2048
// 3.92 -> 3.57; sha256 shape x 1024 2.36 -> 2.26, x 128 1.16 -> 0.93; secp256k1 shape x 64 1.08 -> 0.87 ms per batch.
#define H2V_DEFAULT_LANES 16u
#define H2V_PER_PROOF_LANES 8u
static int ensure_lane(h2v_workspace *w, uint32_t l) {
    if (w->lane[l]) return H2V_OK;
    // the lane's stream and event first, the lane itself last: a lane that exists has both (a failure here leaves lane[l]
    // NULL, and the next call tries again instead of enqueueing on a NULL stream)
    hipStream_t side_st = nullptr;
    if (int rcs = lane_streams(l, &w->lane_st[l], &side_st)) { w->lane_st[l] = nullptr; return rcs; }
    if (!w->lane_ev[l] && !w->mem.event(w->lane_ev[l], hipEventDisableTiming)) return fail(H2V_E_DEVICE, "lane event creation failed");
    h2v_workspace *lw = nullptr;
    int rc = ws_create_for(w->shape, w->device, w->chunk, &lw);
    if (rc) return rc;
    lw->one_stream_mode = 2;            // (set per call: laned_depth)
    lw->pside = side_st;                // (the decompression's stream in the two-stream form: the other half of the lane's pair)
    lw->in_flight_hint = w->in_flight_hint > w->n_lanes ? w->in_flight_hint : w->n_lanes;
    memcpy(lw->opt, w->opt, sizeof lw->opt);
    w->lane[l] = lw;
    return H2V_OK;
}
static int create_lanes_for(const wslayout::Shape &s, int device, uint64_t max_batch, uint32_t n_lanes, uint32_t chunk, h2v_workspace **out) {
    if (max_batch == 0 || max_batch > (1ull << 24)) return fail(H2V_E_ARG, "max_batch out of range");
    if (n_lanes > (uint32_t)h2v_workspace::MAXL) return fail(H2V_E_ARG, "at most 16 lanes");
    // chunk = 0, the library's choice: the plan's own chunk even when max_batch - the largest single call - is smaller: the lanes
    // are what small calls are gathered into (coalesce_call).  An explicit chunk is the caller's, cut to max_batch.
    if (chunk == 0) chunk = lane_chunk();
    else if ((uint64_t)chunk > max_batch) chunk = (uint32_t)max_batch;
    HIPCHK(hipSetDevice(device));
    h2v_workspace *w = new h2v_workspace();
    w->device = device; w->cap = max_batch; w->chunk = chunk;
    w->stride = (uint32_t)((max_batch + 63) / 64 * 64);
    w->shape = s;
    w->lanes_per_proof = n_lanes ? n_lanes : H2V_PER_PROOF_LANES;     // an explicit lane count holds for both modes
    w->n_lanes = n_lanes ? n_lanes : H2V_DEFAULT_LANES;
    w->in_flight_hint = w->n_lanes;
    bool ok = w->mem.event(w->ev_fork, hipEventDisableTiming) && w->mem.alloc(w->accept, wslayout::laned_accept(max_batch));
    // the first lane now (an allocation failure surfaces here, not in the middle of a verify call); the others on first use
    if (ok) ok = ensure_lane(w, 0) == H2V_OK;
    if (!ok) { const std::string e = g_err; ws_release(w); delete w; return fail(H2V_E_DEVICE, "lane creation failed: " + e); }
    reg_add(g_ws_live, w);
    *out = w;
    return H2V_OK;
}
extern "C" int h2v_workspace_create_lanes(const h2v_plan *p, uint64_t max_batch, uint32_t n_lanes, uint32_t chunk, h2v_workspace **out) {
    if (!p || !out) return fail(H2V_E_ARG, "null argument");
    ALIVE(p);
    return create_lanes_for(wslayout::shape_of(p->d, false), p->device, max_batch, n_lanes, chunk, out);
}
// One set of lanes for SEVERAL plans of one device (a node that verifies proofs of several circuits; BASELINE configs[2] names a
// mixed batch): the lane workspaces are sized for the largest of every dimension - MSM terms, point slots, the combiner's
// global register file where a plan needs one, the recursion and fixed-base buffers where a plan has them - so every listed plan
// passes ws_fits, and the calls of all of them go round robin through the SAME lanes and streams.  (One laned workspace per plan
// also works, but their lanes share the pool's sixteen streams pairwise: two plans x 2048 proofs, 6.70 ms per step on two
// workspaces.)
extern "C" int h2v_workspace_create_multi(const h2v_plan *const *plans, uint32_t n_plans, uint64_t max_batch, uint32_t n_lanes, uint32_t chunk, h2v_workspace **out) {
    if (!plans || !out || n_plans == 0) return fail(H2V_E_ARG, "null argument");
    for (uint32_t k = 0; k < n_plans; k++) {
        if (!plans[k]) return fail(H2V_E_ARG, "null plan");
        ALIVE(plans[k]);
        if (plans[k]->device != plans[0]->device) return fail(H2V_E_ARG, "the plans of one workspace must live on one device");
    }
    wslayout::Shape u = wslayout::shape_of(plans[0]->d, false);
    for (uint32_t k = 1; k < n_plans; k++) u = wslayout::shape_union(u, wslayout::shape_of(plans[k]->d, false));
    return create_lanes_for(u, plans[0]->device, max_batch, n_lanes, chunk, out);      // (chunk = 0: the library's lane size, whatever max_batch is)
}
extern "C" int h2v_workspace_create(const h2v_plan *p, uint64_t max_batch, h2v_workspace **out) {
    if (!p || !out) return fail(H2V_E_ARG, "null argument");
    // a workspace for batches of at least four chunks is laned: the call is pipelined inside the library (measured,
    // simple_mul: 8192 proofs in one launch per kernel 5.6 ms per 4096 against 5.9 in two chunks; 20480: 5.3 against 4.7)
    ALIVE(p);
    const wslayout::Shape s = wslayout::shape_of(p->d, false);
    if (max_batch >= 4ull * default_chunk(s)) return h2v_workspace_create_lanes(p, max_batch, 0, 0, out);
    const int rc = ws_create_for(s, p->device, max_batch, out);
    if (rc == H2V_OK) reg_add(g_ws_live, *out);
    return rc;
}
static int option_check(uint32_t option, int32_t value) {
    auto bad = [](const char *m) { return fail(H2V_E_ARG, m); };
    switch (option) {
    case H2V_OPT_MSM_TERMS_PER_LANE: if (value < 0 || value > 4) return bad("terms per lane: 0 (auto) .. 4"); break;
    case H2V_OPT_PAIRING_ENGINE:
        if (!pairing_option_legal(value))
            return bad("pairing engine: 0 (auto), 6, 12, 16, 32, 64 lanes per proof, or 1 (the one-lane cross-check kernel)");
        break;
    case H2V_OPT_STREAMS: if (value < -1 || value > 2) return bad("streams: -1 (auto), 0 (two of the library's), 1 (the caller's), 2 (the caller's + one for the decompression)"); break;
    case H2V_OPT_MSM_LANES_PER_TERM: if (value != 0 && value != 1 && value != 2 && value != 8) return bad("MSM lanes per term: 0 (auto), 1, 2, 8"); break;
    case H2V_OPT_MSM_BLOCK_SIZE: if (value < 0 || value > 512 || value % 64) return bad("MSM block size: 0 (auto), 64 .. 512 in steps of 64"); break;
    case H2V_OPT_MSM_FIXED_SPLIT: if (value < -1 || value > 4) return bad("fixed-base split: 0 (auto), 1 .. 4 bases per lane, -1 (never)"); break;
    case H2V_OPT_COMBINER_SCHEDULE: if (value < 0 || value > 2) return bad("combiner schedule: 0 (auto), 1 (narrow), 2 (wide)"); break;
    case H2V_OPT_COMBINER_PROOFS_PER_BLOCK: if (value < 0 || value > 64 || (value & (value - 1))) return bad("combiner proofs per block: 0 (auto) or a power of two <= 64"); break;
    case H2V_OPT_RLC_GROUP_STAGE: if (value < -1 || value > 0) return bad("RLC group stage: 0 (auto), -1 (off)"); break;
    case H2V_OPT_RLC_WINDOW_BITS: if (value != 0 && (value < 3 || value > (int32_t)PIP_MAX_C)) return bad("RLC window bits: 0 (auto), 3 .. the bucket MSM's maximum"); break;
    case H2V_OPT_RLC_CHAIN: if (value != 0 && (value < 2 || value > 1024)) return bad("RLC entries per lane: 0 (auto), 2 .. 1024"); break;
    case H2V_OPT_RLC_ROUTE: if (value < -1 || value > 0) return bad("RLC routing: 0 (by the observed rate of failing groups), -1 (never)"); break;
    case H2V_OPT_COALESCE: if (value < -1 || value > 0) return bad("coalescing of small calls: 0 (auto: deferred joins, calls of at most half a chunk), -1 (never)"); break;
    default: return bad("unknown option");
    }
    return H2V_OK;
}
extern "C" int h2v_workspace_set_option(h2v_workspace *ws, uint32_t option, int32_t value) {
    if (!ws) return fail(H2V_E_ARG, "null argument");
    ALIVE(ws);
    if (int rc = option_check(option, value)) return rc;
    auto apply = [&](h2v_workspace *w) {
        if (option == H2V_OPT_STREAMS) w->one_stream_mode = value;
        else w->opt[option] = value;
    };
    apply(ws);
    for (uint32_t l = 0; l < (uint32_t)h2v_workspace::MAXL; l++) if (ws->lane[l] && option != H2V_OPT_STREAMS) apply(ws->lane[l]);
    return H2V_OK;
}
extern "C" int h2v_workspace_get_option(const h2v_workspace *ws, uint32_t option, int32_t *value) {
    if (!ws || !value || option == 0 || option >= H2V_OPT_COUNT) return fail(H2V_E_ARG, "bad argument");
    if (option == 9 || option == 10) return fail(H2V_E_ARG, "unknown option");   // (retired ids: include/h2v.h)
    *value = option == H2V_OPT_STREAMS ? ws->one_stream_mode : ws->opt[option];
    return H2V_OK;
}
extern "C" int h2v_workspace_lanes(const h2v_workspace *ws, uint32_t *n_lanes, uint32_t *chunk) {
    if (!ws) return fail(H2V_E_ARG, "null argument");
    if (n_lanes) *n_lanes = ws->n_lanes ? ws->n_lanes : 1;
    if (chunk) *chunk = ws->n_lanes ? ws->chunk : (uint32_t)ws->cap;
    return H2V_OK;
}
static uint32_t laned_depth(const h2v_workspace *w, uint64_t n, bool rlc, int *stream_mode);
extern "C" int h2v_workspace_depth(const h2v_workspace *ws, uint64_t n, int rlc, uint32_t *batches_in_flight) {
    if (!ws || !batches_in_flight) return fail(H2V_E_ARG, "null argument");
    ALIVE(ws);
    *batches_in_flight = ws->n_lanes ? laned_depth(ws, n, rlc != 0, nullptr) : 1;
    return H2V_OK;
}
extern "C" int h2v_workspace_defer_joins(h2v_workspace *ws, int defer) {
    if (!ws) return fail(H2V_E_ARG, "null argument");
    ALIVE(ws);
    if (!ws->n_lanes) return fail(H2V_E_ARG, "only a laned workspace can defer its joins (h2v_workspace_create_lanes)");
    if (!defer) { HIPCHK(hipSetDevice(ws->device)); if (int rcf = co_flush(ws)) return rcf; }   // (an open group of coalesced calls runs now)
    ws->defer_joins = defer != 0;
    return H2V_OK;
}
// Deferred joins and the legacy NULL stream do not go together: the pool streams are created with the default flags
// (hipExtStreamCreateWithCUMask has no non-blocking form), so every operation on the NULL stream - PyTorch's default stream
// IS that stream - waits for all lanes and holds them back behind it: the pipelining would be lost without a word.  A
// deferring workspace therefore refuses stream = NULL (H2V_STREAM_CUMASK=0 streams are non-blocking: allowed).
static int null_stream_check(const h2v_workspace *ws, const void *stream) {
    static const bool blocking_pool = []() { const char *e = getenv("H2V_STREAM_CUMASK"); return !e || atoi(e) != 0; }();
    if (ws && ws->n_lanes && ws->defer_joins && stream == nullptr && blocking_pool)
        return fail(H2V_E_ARG, "a workspace with deferred joins needs a stream of its own: the legacy NULL stream (PyTorch's default stream) is ordered with "
                               "every library stream and would serialise the lanes - pass a non-default stream, or h2v_workspace_defer_joins(ws, 0)");
    return H2V_OK;
}
// An error part of the way through enqueueing a call: work enqueued before it (earlier chunks, the upload from a pinned block)
// may still read the caller's or the workspace's buffers, so nothing may be reused before every stream the workspace may have
// enqueued on has drained.  Returns rc with the error's message.
static int drain_after_error(h2v_workspace *w, int rc) {
    const std::string e = g_err;
    for (hipStream_t q : {w->hs, w->hs_down, w->pmain, w->pside}) if (q) (void)hipStreamSynchronize(q);
    for (uint32_t l = 0; l < w->n_lanes; l++) {
        if (w->lane_st[l]) (void)hipStreamSynchronize(w->lane_st[l]);
        w->lane_busy[l] = false;
    }
    return fail(rc, e);
}
// every lane that has work enqueued since the last join: `st` waits for its last chunk
static int lanes_join(h2v_workspace *w, hipStream_t st, bool host_block = false) {
    if (int rcf = co_flush(w)) return rcf;          // (the open group of coalesced calls runs now)
    for (uint32_t l = 0; l < w->n_lanes; l++)
        if (w->lane_busy[l]) {
            if (host_block) HIPCHK(hipEventSynchronize(w->lane_ev[l]));
            else HIPCHK(hipStreamWaitEvent(st, w->lane_ev[l], 0));
            w->lane_busy[l] = false;
        }
    return H2V_OK;
}
extern "C" int h2v_workspace_join(h2v_workspace *ws, void *stream) {
    if (!ws) return fail(H2V_E_ARG, "null argument");
    ALIVE(ws);
    if (!ws->n_lanes) return H2V_OK;   // an ordinary workspace's calls are already ordered on the caller's stream
    HIPCHK(hipSetDevice(ws->device));
    // stream = NULL: the HOST waits (the legacy NULL stream is never touched: every pool stream is a blocking stream, i.e.
    // ordered with it, and a wait enqueued there would serialise all lanes)
    return lanes_join(ws, (hipStream_t)stream, stream == nullptr);
}
extern "C" void h2v_workspace_free(h2v_workspace *w) {
    if (!w) return;
    reg_del(g_ws_live, w);
    if (!w->dead) ws_release(w);
    delete w;
}
extern "C" int h2v_workspace_hint_in_flight(h2v_workspace *ws, uint32_t n_in_flight) {
    if (!ws || n_in_flight == 0) return fail(H2V_E_ARG, "bad argument");
    ALIVE(ws);
    ws->in_flight_hint = n_in_flight;
    ws->hint_given = true;
    return H2V_OK;
}

// A workspace is sized from the plan it was created for; another plan may use it iff every buffer is large enough for
// it (terms, point slots, a global register file if it needs one, recursion buffers, the fixed-base sum).
static int ws_fits(const h2v_workspace *w, const h2v_plan *p, uint64_t n, bool want_trace) {
    if (w->device != p->device) return fail(H2V_E_ARG, "workspace belongs to another device");
    if (w->cap < n) return fail(H2V_E_ARG, "workspace too small for this batch");
    if (w->n_lanes) {
        if (want_trace) return fail(H2V_E_ARG, "a laned workspace has no trace buffer");
        return ws_fits(w->lane[0], p, n < w->chunk ? n : w->chunk, false);
    }
    const wslayout::Fit f = wslayout::fits(w->shape, wslayout::shape_of(p->d, true), want_trace);
    return f == wslayout::Fit::OK ? (int)H2V_OK : fail(H2V_E_ARG, wslayout::fit_message(f));
}

// Library-owned streams.  The runtime multiplexes ordinary streams onto GPU_MAX_HW_QUEUES (default 4) hardware queues per
// process, and kernels of two streams that share a queue run one after the other - with five batches in flight on three
// streams each that is the difference between 5.7 and 4.3 ms per 4096-proof batch (round 2 needed GPU_MAX_HW_QUEUES=16 in
// the caller's environment for it).  A stream created with an explicit CU mask gets a hardware queue of its own, whatever
// the process-wide setting is (measured, default environment: 5 lanes 5.79 -> 4.34 ms per batch).  Every queue also gets
// its own scratch arena, sized for the kernel with the largest private segment (a process that had created 47 of them
// died with HSA_STATUS_ERROR_OUT_OF_RESOURCES at the next launch), so the library owns a fixed POOL of such streams per
// device - H2V_QUEUE_POOL, default 16 (24 measured slower: 4.97 against 4.30 ms per batch) - and hands them out round robin: workspaces share them (a stream is an ordering
// domain, sharing one only adds order), they live until h2v_shutdown, and the mask names every CU.  Pool streams have the
// default flags, i.e. they are ordered with the legacy NULL stream: callers that defer joins should not submit on the
// NULL stream.  H2V_STREAM_CUMASK=0: plain non-blocking streams of the runtime's own pool instead.
static std::vector<hipStream_t> g_pool[16];
static size_t g_pool_next[16] = {};
extern "C" int h2v_shutdown(int device);
static const size_t g_pool_cap = []() { const char *e = getenv("H2V_QUEUE_POOL"); const int v = e ? atoi(e) : 16; return (size_t)(v < 1 ? 1 : v > 32 ? 32 : v); }();
static hipError_t make_stream(hipStream_t *s) {
    static const int cumask = []() { const char *e = getenv("H2V_STREAM_CUMASK"); return e ? atoi(e) : 1; }();
    const size_t pool_cap = g_pool_cap;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 16) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(g_reg_mu);
    if (g_shut[dev]) return hipErrorContextIsDestroyed;
    if (g_pool[dev].size() < pool_cap) {
        hipStream_t ns = nullptr;
        if (cumask) {
            int cus = 256;
            (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
            std::vector<uint32_t> mask((cus + 31) / 32, 0xffffffffu);
            if (cus % 32) mask.back() = (1u << (cus % 32)) - 1;
            e = hipExtStreamCreateWithCUMask(&ns, (uint32_t)mask.size(), mask.data());
        } else {
            e = hipStreamCreateWithFlags(&ns, hipStreamNonBlocking);
        }
        if (e != hipSuccess) return e;
        // registered now, i.e. after the HIP runtime has initialised itself: exit handlers run in reverse order of
        // registration, so the pool is destroyed while the runtime (and a profiler's tool) are still whole
        static const int registered = atexit([]() { (void)h2v_shutdown(-1); });
        (void)registered;
        g_pool[dev].push_back(ns);
        *s = ns;
        return hipSuccess;
    }
    *s = g_pool[dev][g_pool_next[dev]++ % g_pool[dev].size()];
    return hipSuccess;
}
// The two streams of lane l of ANY laned workspace: a fixed place in the pool, so that the lanes of one workspace never share a
// stream among themselves whatever else was created in between (handing streams out in creation order, two workspaces whose
// lanes were created alternately ended up with a lane whose side stream WAS its main stream, and with two lanes of one
// workspace on one pair: 3.7 / 4.1 ms per call where 3.3 / 3.4 are normal - bench.py's mixed workload, round 4).  Lanes 0..7
// (the per-proof mode's eight two-stream lanes): main 2 l, side 2 l + 1; lanes 8..15 (only the sixteen one-stream lanes of
// small chunks and of the RLC mode reach them): the odd streams as main.  Lanes of different workspaces with the same index
// share their pair - with sixteen hardware queues and two plans in flight something has to.  (main l, side l + 8 instead: 1.7 % slower,
// 3.30-3.32 against 3.24-3.26 ms per simple_mul x 4096 batch; pairs spread over the pool in steps of four: the same.)
static int lane_streams(uint32_t l, hipStream_t *main_st, hipStream_t *side_st) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    for (;;) {                                     // fill the pool (make_stream creates while it is below its capacity)
        size_t have, cap;
        { std::lock_guard<std::mutex> lock(g_reg_mu); have = g_pool[dev].size(); cap = g_pool_cap; }
        if (have >= cap && have > 0) break;
        hipStream_t q;
        if (make_stream(&q) != hipSuccess) return fail(H2V_E_DEVICE, "lane stream creation failed");
        { std::lock_guard<std::mutex> lock(g_reg_mu); if (g_pool[dev].size() == have) break; }   // (H2V_QUEUE_POOL smaller than asked: the pool is full)
    }
    std::lock_guard<std::mutex> lock(g_reg_mu);
    const size_t n = g_pool[dev].size();
    if (n == 0) return fail(H2V_E_DEVICE, "no pool stream");
    const uint32_t m = l < 8 ? 2 * l : 2 * (l - 8) + 1;
    *main_st = g_pool[dev][m % n];
    *side_st = g_pool[dev][(m ^ 1u) % n];
    return H2V_OK;
}
// Releases everything the library owns on `device` (-1: on every device): waits for the pool streams, releases every live
// workspace (they become empty shells: dead) and every plan's device memory, destroys the pool streams.  Idempotent.
extern "C" int h2v_shutdown(int device) {
    if (device < -1 || device >= 16) return fail(H2V_E_ARG, "device index out of range");
    std::vector<h2v_workspace *> wss;
    std::vector<h2v_plan *> plans;
    std::vector<hipStream_t> streams[16];
    {
        std::lock_guard<std::mutex> lock(g_reg_mu);
        for (h2v_workspace *w : g_ws_live) if (!w->dead && (device < 0 || w->device == device)) wss.push_back(w);
        for (h2v_plan *p : g_plan_live) if (!p->dead && (device < 0 || p->device == device)) plans.push_back(p);
        for (int d = 0; d < 16; d++)
            if (device < 0 || d == device) { g_shut[d] = true; streams[d].swap(g_pool[d]); }
    }
    int rc = H2V_OK;
    for (int d = 0; d < 16; d++) {
        if (streams[d].empty()) continue;
        if (hipSetDevice(d) != hipSuccess) { rc = fail(H2V_E_DEVICE, "hipSetDevice failed during shutdown"); continue; }
        for (hipStream_t q : streams[d]) (void)hipStreamSynchronize(q);
    }
    for (h2v_workspace *w : wss) {
        const int dev = w->device;
        ws_release(w);
        *w = h2v_workspace();
        w->device = dev; w->dead = true;
    }
    for (h2v_plan *p : plans) { plan_release(p); p->dead = true; }
    for (int d = 0; d < 16; d++) {
        if (streams[d].empty()) continue;
        if (hipSetDevice(d) != hipSuccess) continue;
        for (hipStream_t q : streams[d])
            if (hipStreamDestroy(q) != hipSuccess) rc = fail(H2V_E_DEVICE, "hipStreamDestroy(pool stream) failed");
    }
    return rc;
}
// the main / side stream of the pipeline, created when first asked for
static int ws_streams(h2v_workspace *w, bool need_main, bool need_side) {
    if (need_main && !w->pmain) HIPCHK(make_stream(&w->pmain));
    if (need_side && !w->pside) HIPCHK(make_stream(&w->pside));
    return H2V_OK;
}

// launch-shape options of the workspace a call runs on (h2v_workspace_set_option): the launchers below run on the calling
// host thread, inside run_pipeline / run_rlc, which set this for their duration
struct LaunchOptions { int32_t v[H2V_OPT_COUNT] = {}; uint32_t in_flight = 1; };
static thread_local LaunchOptions g_opts;
static thread_local LaunchOptions g_probe_opts;     // h2v_probe_set_option: the shape options the probes of this thread launch with
// the launch options of workspace w while a call's kernels are enqueued on this thread
struct LaunchOptsScope {
    explicit LaunchOptsScope(const h2v_workspace *w) { memcpy(g_opts.v, w->opt, sizeof g_opts.v); g_opts.in_flight = w->in_flight_hint; }
    ~LaunchOptsScope() { g_opts = LaunchOptions(); }
};
struct ProbeOpts { ProbeOpts() { g_opts = g_probe_opts; } ~ProbeOpts() { g_opts = LaunchOptions(); } };
extern "C" int h2v_probe_set_option(uint32_t option, int32_t value) {
    if (option == H2V_OPT_STREAMS) return fail(H2V_E_ARG, "the probes run on the NULL stream");
    if (int rc = option_check(option, value)) return rc;
    g_probe_opts.v[option] = value;
    return H2V_OK;
}
// Transcript + combiner launch.  A block is one wave; its 64 lanes are P proofs x L lanes per proof (the plan's
// bundles have L records), the Fr register file of the P proofs lives in LDS (160 KB per CU).  A single-lane plan whose
// register file does not fit 64 proofs runs P = 32 / 16 / 8 proofs per block with the other lanes idle, or - below 8 -
// with the register file in the workspace's global buffer.
static int launch_vm(const H2vDevPlan &d0, uint32_t n, uint32_t stride, const uint8_t *proofs, const uint64_t *off, const uint8_t *inst,
                     const uint8_t *ci, uint32_t *regs, uint32_t *scalars, uint32_t *status, uint32_t *trace, hipStream_t st) {
    // The wide schedule (more lanes per proof: shorter chain, more waves) when the launch would leave most of the chip
    // idle anyway - at most a quarter of the SIMDs get a wave - and nobody asked for the trace (its register numbers are
    // the narrow schedule's).  H2V_OPT_COMBINER_SCHEDULE forces the choice.
    const int env_wide = g_opts.v[H2V_OPT_COMBINER_SCHEDULE] - 1;   // -1 auto, 0 narrow, 1 wide
    H2vDevPlan d = d0;
    const bool wide_ok = d.wide_lanes && !trace;
    // (eight or more batches in flight: the chip is full anyway and the wide schedule's extra instructions count - only launches
    //  of at most 32 waves take it.  ms per batch, wide -> narrow schedule: sha256 shape x 128 0.66 -> 0.69, x 256 0.88 -> 0.84,
    //  x 512 1.22 -> 1.18, x 1024 2.16 -> 2.00; secp256k1 shape x 64 0.54 -> 0.56, x 512 1.32 -> 1.16)
    const uint64_t wide_waves = ((uint64_t)n * d.wide_lanes + 63) / 64;
    const bool wide = wide_ok && (env_wide >= 0 ? env_wide != 0 : wide_waves <= (g_opts.in_flight >= 8 ? 32u : 256u));
    if (wide) { d.vm_lanes = d.wide_lanes; d.n_regs = d.wide_n_regs; d.n_instr = d.wide_n_instr; d.instr = d.wide_instr; }
    // the kernels are instantiated per transcript hash (a compile-time choice inside them): the plan's kind picks
    const bool b512 = d.tr_kind == H2V_TR_BLAKE2B_512;
    if (d.tr_kind >= H2V_TR_KIND_COUNT) return fail(H2V_E_PLAN, "no combiner kernel for this transcript hash");
    uint32_t P = vm_lds_slots(d);
    if (P == 0) {
        const auto k_glb = b512 ? k_transcript_combiner_b512 : k_transcript_combiner;
        hipLaunchKernelGGL(k_glb, dim3((n + 63) / 64), dim3(64), 0, st, d, n, stride, proofs, off, inst, ci, regs, scalars, status, trace);
        return H2V_OK;
    }
    // Fewer proofs per block than the wave could serve (the spare lanes shadow): the register file of P proofs is what
    // decides how many blocks a CU holds (simple_mul, P = 32: 79 + 8 KB = ONE block per CU = one wave on one of its four
    // SIMDs), and a wave's chain is as long with 16 proofs as with 32.  H2V_OPT_COMBINER_PROOFS_PER_BLOCK forces P.
    const int env_p = g_opts.v[H2V_OPT_COMBINER_PROOFS_PER_BLOCK];
    if (env_p >= 1 && (env_p & (env_p - 1)) == 0 && (uint32_t)env_p <= P) P = (uint32_t)env_p;
    const size_t lds = (size_t)d.n_regs * 32 * P;
    const auto k_lds = b512 ? k_transcript_combiner_lds_b512 : k_transcript_combiner_lds;
    HIPCHK(hipFuncSetAttribute((const void *)k_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_lds, dim3((n + P - 1) / P), dim3(64), lds, st, d, n, P, proofs, off, inst, ci, scalars, status, trace);
    return H2V_OK;
}

// MSM launch geometry: the shape model is host-only code of its own (h2v_msm_shape.hpp: lanes per term, block size, segments,
// fixed-base split, terms per lane); this file gives it the device's SIMD count and the H2V_OPT_MSM_* options and launches
// what it decides.  LDS: MSM_LDS_BYTES (h2v_msm.hpp, next to the reduction whose layout it is).
static double msm_n_simd() {
    static const double v = []() {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
        return 4.0 * cus;
    }();
    return v;
}
static MsmModel msm_model() {
    return {msm_n_simd(), g_opts.v[H2V_OPT_MSM_LANES_PER_TERM], (uint32_t)g_opts.v[H2V_OPT_MSM_BLOCK_SIZE], g_opts.v[H2V_OPT_MSM_TERMS_PER_LANE],
            g_opts.v[H2V_OPT_MSM_FIXED_SPLIT]};
}
// The partial-sum buffer of segmented launches: [segment][proof][36 dwords], room for max_seg segments of the launch's proofs.
// parts == NULL: the launch may not be segmented.
struct SegBuf {
    uint32_t *parts = nullptr; uint32_t max_seg = 0;
    uint32_t room() const { return parts ? max_seg : 0u; }   // (what the shape model takes)
};
// The one-group range of a term table: terms [term_base, term_base + n_terms), their scalars from column col_base on of
// scal_stride per proof, summed into `out`.  pt_tab: the per-proof window tables, or NULL (every lane builds its own).
static H2vMsmArgs msm_args(const H2vDevPlan &d, uint32_t term_base, uint32_t n_terms, uint32_t scal_stride, uint32_t col_base, uint32_t slots,
                           uint32_t *out, const uint32_t *pt_tab) {
    H2vMsmArgs a = {};
    a.terms = d.terms; a.term_base = term_base; a.n_terms = n_terms; a.scal_stride = scal_stride; a.scal_col_base = col_base; a.slots = slots;
    a.grp_end[0] = a.grp_end[1] = a.grp_end[2] = n_terms;
    a.out[0] = out;
    a.pt_tab = pt_tab; a.vk_tab = d.vk_tab;
    return a;
}
// ... of the plan's VK-base terms through the all-window tables, k bases per lane (k_g1_msm_fixed)
static H2vMsmArgs msm_fixed_args(const H2vDevPlan &d, uint32_t scal_stride, uint32_t col_base, uint32_t *out, const uint32_t *pt_tab, uint32_t k) {
    H2vMsmArgs a = msm_args(d, d.n_var, d.n_fix, scal_stride, col_base, H2V_SLOTS(d), out, pt_tab);
    a.fix_tab = d.fix_tab; a.fix_k = k; a.n_fixl = (d.n_fix + k - 1) / k;
    return a;
}
static void launch_msm_fixed(const H2vDevPlan &d, const H2vMsmArgs &mf, uint32_t n, uint32_t bs, const uint32_t *scalars, const uint32_t *pts, hipStream_t st) {
    const uint32_t pbf = bs / mf.n_fixl;
    hipLaunchKernelGGL(k_g1_msm_fixed, dim3((n + pbf - 1) / pbf), dim3(bs), MSM_LDS_BYTES(bs), st, d, mf, n, pbf, scalars, pts, (uint32_t *)nullptr);
}
// the eight ladder entry points (h2v_msm.hpp: msm_ladder_entry, MSM_COND_BODY); the unsegmented ones take no (seg_terms, parts)
typedef void (*MsmLadderKernel)(H2vDevPlan, H2vMsmArgs, uint32_t, uint32_t, const uint32_t *, const uint32_t *, uint32_t *);
typedef void (*MsmSegKernel)(H2vDevPlan, H2vMsmArgs, uint32_t, uint32_t, uint32_t, uint32_t *, const uint32_t *, const uint32_t *, uint32_t *);
static MsmLadderKernel msm_ladder_kernel(uint32_t lpt, bool cond) {
    static const MsmLadderKernel tab[2][2] = {{k_g1_msm, k_g1_msm_cond}, {k_g1_msm_merged, k_g1_msm_merged_cond}};
    return lpt == 8 && !cond ? k_g1_msm_quad : tab[lpt == 1][cond];   // (the quad has no conditional form; its shape is never chosen for a launch with ma.skip)
}
static MsmSegKernel msm_seg_kernel(uint32_t lpt, bool cond) {
    static const MsmSegKernel tab[2][2] = {{k_g1_msm_seg, k_g1_msm_cond_seg}, {k_g1_msm_merged_seg, k_g1_msm_merged_cond_seg}};
    return tab[lpt == 1][cond];
}
// The ladder launch of a range in the shape `sh`.  The segmented form of a one-group range (sh.n_seg > 1): one segment per
// blockIdx.y into seg.parts, then the fold into ma.out[0] on the same stream.  ma.skip (fall-back of the RLC batch mode): a grid
// of at most one block per CU - over all segments - walks the logical blocks.
// returns the lanes per term launched, 0 if nothing was launched (no shape fits: see msm_ladder_shape)
static uint32_t launch_msm_ladders(const H2vDevPlan &d, const H2vMsmArgs &ma, uint32_t n, const MsmShape &sh, const uint32_t *scalars,
                                   const uint32_t *pts, uint32_t *tabws, hipStream_t st, const SegBuf &seg = SegBuf()) {
    const bool segmented = sh.n_seg > 1;
    if (segmented) {
        if (!seg.parts || sh.n_seg > seg.max_seg || !ma.pt_tab || ma.grp_end[0] != ma.n_terms || sh.lpt > 2) return 0;
        if (sh.bs < sh.lpt * sh.seg_terms || (uint64_t)sh.seg_terms * (sh.n_seg - 1) >= ma.n_terms) return 0;
    } else if (sh.bs == 0 || sh.lpt * ma.n_terms > sh.bs) {
        return 0;
    }
    const uint32_t per_block = sh.bs / (sh.lpt * (segmented ? sh.seg_terms : ma.n_terms));
    const uint32_t blocks = (n + per_block - 1) / per_block, cg = ((uint32_t)(msm_n_simd() / 4.0) + sh.n_seg - 1) / sh.n_seg;
    const dim3 grid(ma.skip && cg < blocks ? cg : blocks, sh.n_seg);
    if (segmented) {
        hipLaunchKernelGGL(msm_seg_kernel(sh.lpt, ma.skip != nullptr), grid, dim3(sh.bs), MSM_LDS_BYTES(sh.bs), st, d, ma, n, per_block, sh.seg_terms, seg.parts, scalars, pts, tabws);
        hipLaunchKernelGGL(k_g1_sum_segments, dim3((n + 63) / 64), dim3(64), 0, st, n, sh.n_seg, (const uint32_t *)seg.parts, ma.out[0], ma.skip);
    } else {
        hipLaunchKernelGGL(msm_ladder_kernel(sh.lpt, ma.skip != nullptr), grid, dim3(sh.bs), MSM_LDS_BYTES(sh.bs), st, d, ma, n, per_block, scalars, pts, tabws);
    }
    return sh.lpt;
}
static uint32_t launch_msm_range(const H2vDevPlan &d, const H2vMsmArgs &ma, uint32_t n, const uint32_t *scalars, const uint32_t *pts,
                                 uint32_t *tabws, hipStream_t st, uint32_t in_flight_hint = 1, const SegBuf &seg = SegBuf()) {
    const MsmModel m = msm_model();
    const int tpl = msm_terms_per_lane(m, in_flight_hint, n, ma.n_terms);
    // (only launches of at least a quarter of a wave per SIMD at one lane per term: below that the launch is a chain of lone
    //  waves whatever else is in flight, and the two-lanes-per-term ladder is the shortest chain - sha256 shape x 128 with six
    //  shares in flight: MSM 2.5 ms -> 1.4 ms alone)
    // (eight or more batches in flight: from an eighth - sha256 / secp256k1 shape x 256, sixteen shares in flight: 1.05 / 1.08 ->
    //  0.89 / 0.91 ms per share with two terms per lane; x 128 and x 64 stay with the shortest chain: 0.66 -> 0.74, 0.54 -> 0.64)
    const bool fills = (double)n * ma.n_terms / 64.0 >= msm_n_simd() / (in_flight_hint >= 8 ? 8.0 : 4.0);
    const bool tpl_forced = m.terms_per_lane > 0;
    if (tpl > 1 && (fills || tpl_forced) && ma.pt_tab && !ma.skip && ma.grp_end[0] == ma.n_terms && ma.n_terms >= (uint32_t)tpl && ma.n_terms <= 256u * tpl) {
        // (h2v_msm_shape.hpp: the proof's 2 T GLV halves dealt out evenly over the lanes)
        const MsmMultiShape ms = msm_multi_shape(ma.n_terms, tpl, tpl_forced);
        const uint32_t bs = 256, hpl = ms.hpl;
        const uint32_t per_block = bs / ms.lpp, blocks = (n + per_block - 1) / per_block;
        hipLaunchKernelGGL(k_g1_msm_multi, dim3(blocks), dim3(bs), MSM_LDS_BYTES(bs), st, d, ma, n, per_block, hpl, scalars, pts, tabws);
        return 16 + (hpl + 1) / 2;   // reported as msm_lanes_per_term: 18 / 19 / 20 = up to two / three / four terms' halves per lane
    }
    // (segments: one-group ranges with prebuilt window tables only)
    const SegBuf sg = ma.pt_tab && ma.grp_end[0] == ma.n_terms ? seg : SegBuf();
    return launch_msm_ladders(d, ma, n, msm_ladder_shape(m, ma.n_terms, n, 0.0, ma.pt_tab != nullptr && !ma.skip, sg.room()), scalars, pts, tabws, st, sg);
}
// the proof's own MSM: terms [0, n_main_terms) of the plan's table, scalars from the combiner, points from decompression.
// A recursive plan sums acc_left and acc_right + fixed bases in the same launch (three groups, three outputs).
// Recursive plans with a sum of more than 64 terms take the three-group launch only when its lanes fit one block; otherwise the
// three sums run as separate ranges one after the other on the stream, each segmented where it needs to be and each with the
// caller's in-flight hint (the multi-term form where it applies).
// Returns the lanes per term launched - of the proof's own sum when the ranges run separately - or 0: nothing launched.
static uint32_t launch_msm(const H2vDevPlan &d, uint32_t n, const uint32_t *scalars, const uint32_t *pts, const uint32_t *pt_tab,
                       uint32_t *er, uint32_t *accl, uint32_t *accr, hipStream_t st, uint32_t in_flight_hint = 1, const SegBuf &seg = SegBuf()) {
    H2vMsmArgs ma = msm_args(d, 0, d.n_main_terms, d.n_terms, 0, H2V_SLOTS(d), er, pt_tab);
    if (d.ivc) {
        if (msm_sum_width(d) > 64 && msm_ladder_fit(msm_model(), d.n_terms, n, 0.0, pt_tab != nullptr).cost == 1e300) {
            const uint32_t m = d.n_main_terms;
            const H2vMsmArgs ranges[3] = {
                ma,
                msm_args(d, m, 1, d.n_terms, m, H2V_SLOTS(d), accl, pt_tab),
                msm_args(d, m + 1, d.n_terms - m - 1, d.n_terms, m + 1, H2V_SLOTS(d), accr, pt_tab)};
            uint32_t code = 0;
            for (const H2vMsmArgs &r : ranges) {
                const uint32_t c = launch_msm_range(d, r, n, scalars, pts, nullptr, st, in_flight_hint, seg);
                if (!c) return 0;
                if (!code) code = c;
            }
            return code;
        }
        ma.n_terms = d.n_terms;
        ma.grp_end[0] = d.n_main_terms; ma.grp_end[1] = d.n_main_terms + 1; ma.grp_end[2] = d.n_terms;
        ma.out[1] = accl; ma.out[2] = accr;
    }
    return launch_msm_range(d, ma, n, scalars, pts, nullptr, st, in_flight_hint, seg);
}
// Recursion (IVC) fold between the MSM and the pairing (emitters/aiken.rs:696-757): the batching challenge from
// (el, er, acc_left, acc_right_final), then el' = el + c acc_left and er' = er + c acc_right_final in one two-group
// launch over the fold's own point / scalar buffers.  Pointers are the chunk's.
struct IvcBufs { uint32_t *accl, *accr, *fold_pts, *fold_scal, *el2, *er2; };
static void launch_ivc_fold(const H2vDevPlan &d, uint32_t n, const uint32_t *pts, const uint32_t *er,
                            const IvcBufs &b, uint32_t *tabws, hipStream_t st) {
    hipLaunchKernelGGL(k_ivc_challenge, dim3((n + 63) / 64), dim3(64), 0, st, d, n, pts, er, b.accl, b.accr, b.fold_pts, b.fold_scal);
    H2vMsmArgs fold = msm_args(d, 0, 4, 4, 0, 4, b.el2, nullptr);   // two groups of two terms over the fold's own table
    fold.terms = d.fold_terms; fold.vk_tab = nullptr;
    fold.grp_end[0] = 2; fold.out[1] = b.er2;
    launch_msm_range(d, fold, n, b.fold_scal, b.fold_pts, tabws, st);
}
// The per-proof pairing: ONE launch site for the six engines.  Which engine runs, and on what grid, is h2v_pairing_engine.hpp's
// answer (the engine table, the rule and the measurements behind its thresholds); here are the table's kernels and their LDS bytes.
// skip != NULL: the conditional form, the fall-back of a batch check - the normal engine on its walking grid, every block of which
// returns at once when *skip != 0.  probe_impl: h2v_probe_pairing_states' impl (its hint: PAIRING_HINT_PROBE); the pipelines'
// launches are the rule under the workspace's option, which is what the probes call impl 1.
// Returns the lanes per proof of the engine that ran (h2v_timings.pairing_lanes_per_proof, the probes' lanes_out).
typedef void (*PairingKernel)(H2vDevPlan, uint32_t, const uint32_t *, const uint8_t *, const uint8_t *, const uint32_t *, const uint32_t *, uint32_t *, uint8_t *, uint32_t *);
typedef void (*PairingKernelSkip)(H2vDevPlan, uint32_t, const uint32_t *, const uint8_t *, const uint8_t *, const uint32_t *, const uint32_t *, uint32_t *, uint8_t *, uint32_t *, const uint32_t *);
// k_pairing_coop alone takes the skip pointer, as its last argument: the launch below hands every kernel the same argument list, of
// which a kernel reads as many as it has parameters.  That erases the kernels' types, so a kernel gets into the table only through
// pairing_kernel(): an implicit conversion to one of the two signatures, which does not compile for a kernel with other parameters.
static const void *pairing_kernel(PairingKernel k) { return (const void *)k; }
static const void *pairing_kernel(PairingKernelSkip k) { return (const void *)k; }
struct PairingLaunchRow { const void *kernel; size_t lds; };
static const PairingLaunchRow PAIRING_LAUNCH[PE_COUNT] = {
    {pairing_kernel(k_pairing_check), 0},
    {pairing_kernel(k_pairing_six), SIX_LDS_BYTES},
    {pairing_kernel(k_pairing_coop_twelve), COOP_LDS_BYTES(COOP_GROUPS_TWELVE)},
    {pairing_kernel(k_pairing_coop_narrow), COOP_LDS_BYTES(COOP_GROUPS_NARROW)},
    {pairing_kernel(k_pairing_coop), COOP_LDS_BYTES(COOP_GROUPS_PER_WAVE)},
    {pairing_kernel(k_pairing_coop_wide), COOP_LDS_BYTES(1)},
};
static_assert(PAIRING_ENGINES[PE_ONE_LANE].per_wave == 64 && PAIRING_ENGINES[PE_SIX].per_wave == SIX_GROUPS &&
              PAIRING_ENGINES[PE_TWELVE].per_wave == COOP_GROUPS_TWELVE && PAIRING_ENGINES[PE_NARROW].per_wave == COOP_GROUPS_NARROW &&
              PAIRING_ENGINES[PE_COOP32].per_wave == COOP_GROUPS_PER_WAVE && PAIRING_ENGINES[PE_WIDE].per_wave == 1,
              "h2v_pairing_engine.hpp: proofs per wave are the kernels' group counts");
static uint32_t launch_pairing(const H2vDevPlan &d, uint32_t n, const uint32_t *pts, const uint8_t *valid, const uint8_t *valid_sub, const uint32_t *er,
                               const uint32_t *el_jac, uint32_t *status, uint8_t *accept, uint32_t *dbg, hipStream_t st, uint32_t in_flight_hint = 1,
                               const uint32_t *skip = nullptr, int probe_impl = PAIRING_IMPL_RULE) {
    const double S = msm_n_simd();
    const PairingEngine e = skip ? PE_COOP32 : pairing_engine(S, g_opts.v[H2V_OPT_PAIRING_ENGINE], n, in_flight_hint, d.six_norm28 != nullptr, probe_impl);
    const uint32_t grid = skip ? pairing_grid_behind(S, n) : pairing_grid(e, n);
    void *args[] = {(void *)&d, &n, &pts, &valid, &valid_sub, &er, &el_jac, &status, &accept, &dbg, &skip};
    (void)hipLaunchKernel(PAIRING_LAUNCH[e].kernel, dim3(grid), dim3(64), args, PAIRING_LAUNCH[e].lds, st);   // (errors: the callers' hipGetLastError)
    return (uint32_t)PAIRING_ENGINES[e].option;
}

// ---------------------------------------------------------------------------------------------- pipeline
// Enqueues the four kernels.  The decompression kernel (many short waves) runs on a side stream beside the
// transcript+combiner kernel (few long waves), and the two join before the MSM.
extern "C" int h2v_workspace_timings(h2v_workspace *w, uint32_t calls_back, h2v_timings *tm);
// ---- one unit of work on one ordinary workspace (or lane): its kind and its buffers, nothing else
//   VERIFY       the four kernels; accept[] and (optional) status[]
//   PREPARE      instead of the pairing, k_prepare_export writes each proof's pair compress(L) || compress(R) to pairs_out
//                (n x 24 dwords) and the status words without H2V_ST_PAIRING; accept is not written
//   CHECK        the pairing alone over n x 96 bytes of `pairs` (run_check)
//   RLC          the batch check over the proofs, the per-proof kernels behind its skip flags (run_rlc)
//   PAIR_RLC     the batch check over `pairs` (run_pairs_rlc)
//   FOLD_RLC     H2V_RLC_FOLD_PAIRS, recursive plans: instead of the per-proof pairing, the batch check over the folded pairs
//                (fold_pairs_tail)
//   ROUTED       an RLC call sent straight to the per-proof kernels (run_routed)
//   MIXED_SUB    h2v_verify_mixed, a per-plan sub-batch: instead of the pairing, k_mixed_pairs writes each proof's pair, `good`
//                and its pre-pairing status at pos[i] - its position in the call - of the call's pool; the record is a prepare call's
//   MIXED_TAIL / MIXED_TAIL_RLC   the pairing / the batch check over the call's pool (run_mixed_tail)
//   MIXED_SUB_TERMS   H2V_MIXED_FOLD_MSM, a sub-batch of a plan that has the batch form: phase 1 alone, then k_mixed_terms writes the
//                proofs' terms into the call's term pool (run_mixed_terms); no MSM, no pair; the record is a prepare call's
//   MIXED_FOLD_TAIL   H2V_MIXED_FOLD_MSM: ONE bucket MSM over the call's term pool and ONE pairing (run_mixed_fold_tail)
//   MIXED_ACROSS_TAIL   H2V_MIXED_ACROSS_SRS without the fold form: the batch check over the call's pool with one left-hand sum per
//                SRS class and ONE multi-pairing, the per-pair kernels class by class behind it (run_across_tail)
//   MIXED_GROUP  H2V_MIXED_GROUPED: MIXED_SUB_TERMS for a range of the grouped positions - every groupable plan's share of it in ONE
//                launch per kernel (run_mixed_group); n / first: the range's size and first grouped position
// seed: the batch coefficients' (RLC kinds).  fail_ctr: where a failed batch check is counted - a lane's chunk or a coalesced
// group: its parent's word; NULL (a call of its own): its record's word, zeroed by the call.
enum class UnitKind : uint8_t { VERIFY, PREPARE, CHECK, RLC, PAIR_RLC, FOLD_RLC, ROUTED, MIXED_SUB, MIXED_TAIL, MIXED_TAIL_RLC, MIXED_SUB_TERMS, MIXED_FOLD_TAIL, MIXED_GROUP, MIXED_ACROSS_TAIL };
struct MixedFold;
// the pool of a mixed call, caller's order: pairs (two-slot affine records), good_i, 2 x cap bytes of 1 (the `valid` of a two-slot
// view) and the status words (pre-pairing bits; the tail folds H2V_ST_PAIRING in)
struct MixedPool { uint32_t *pool; uint8_t *good; const uint8_t *ones; uint32_t *status; };
struct Unit {
    UnitKind kind;
    const h2v_plan *p;
    uint32_t n;
    const uint8_t *proofs = nullptr; const uint64_t *off = nullptr; const uint8_t *inst = nullptr, *ci = nullptr;
    const uint8_t *pairs = nullptr;
    uint8_t *accept = nullptr; uint32_t *status = nullptr; uint8_t *pairs_out = nullptr;
    MixedPool pool = {}; const uint32_t *pos = nullptr;
    const MixedFold *fold = nullptr;   // H2V_MIXED_FOLD_MSM: the call's term pool and its layout; fold_plan: the unit's plan in the call's
    uint32_t fold_plan = 0, first = 0; // list; first: the unit's first proof within its plan's sub-batch (slice)
    uint32_t seed[8] = {};
    // H2V_RLC_SEED_TRANSCRIPT: derive (the entry points set it, on batch-check kinds only) asks run_call for a derived seed; it
    // sets seed_dev - the call's slot of the workspace's seed ring, which the coefficient kernels then read in place of `seed` -
    // and run_chunks the chunk's tweak of its word 7.  The form of the rule follows the kind (PAIR_RLC: pairs).  route: run_call's
    // routing decision for an RLC call over proofs (a routed call derives nothing)
    bool derive = false, route = false;
    const uint32_t *seed_dev = nullptr;
    uint32_t seed_xor7 = 0;
    uint32_t *fail_ctr = nullptr;
    bool one_stream_opt = false;       // RLC: h2v_rlc_opts.flags & H2V_RLC_ONE_STREAM (lanes and coalesced groups: always)
    bool trace = false;                // h2v_trace: the combiner's intermediate values to the workspace's trace buffer
    // an AGGREGATE call (h2v_aggregate_batch / _mixed; kinds RLC, FOLD_RLC, MIXED_FOLD_TAIL): instead of the batch pairing and what
    // is queued behind it, the unit's two sums go to part `part` of agg_parts (its chunk number: run_chunks) and good_i to accept[],
    // which is the caller's included[] (agg_chunk)
    uint32_t *agg_parts = nullptr;
    uint32_t part = 0;
    bool batch_check() const { return kind == UnitKind::RLC || kind == UnitKind::PAIR_RLC || kind == UnitKind::FOLD_RLC || kind == UnitKind::MIXED_TAIL_RLC; }
    // the same unit for proofs / pairs lo .. lo + m (proof offsets are absolute: `proofs` stays; a sub-batch writes the pool
    // through pos[], the tail reads its own part of it)
    Unit slice(uint32_t lo, uint32_t m) const {
        Unit c = *this;
        c.n = m;
        if (off) c.off = off + lo;
        if (inst) c.inst = inst + (size_t)lo * p->d.n_pi * 32;
        if (ci) c.ci = ci + (size_t)lo * 48;
        if (pairs) c.pairs = pairs + (size_t)lo * 96;
        if (accept) c.accept = accept + lo;
        if (status) c.status = status + lo;
        if (pairs_out) c.pairs_out = pairs_out + (size_t)lo * 96;
        if (pos) c.pos = pos + lo;
        c.first = first + lo;
        if (kind == UnitKind::MIXED_TAIL || kind == UnitKind::MIXED_TAIL_RLC) c.pool = {pool.pool + (size_t)lo * 48, pool.good + lo, pool.ones, pool.status + lo};
        return c;
    }
};
// the eight words of a call's seed; src == NULL: zeros
static void copy_seed(uint32_t dst[8], const uint32_t *src) {
    for (int q = 0; q < 8; q++) dst[q] = src ? src[q] : 0;
}
static Unit unit_of_batch(UnitKind kind, const h2v_plan *p, const h2v_batch *b, uint8_t *accept, uint32_t *status) {
    Unit u{kind, p, (uint32_t)b->n};
    u.proofs = b->proofs; u.off = b->proof_off; u.inst = b->instances; u.ci = b->committed;
    u.accept = accept; u.status = status;
    return u;
}
static Unit unit_of_pairs(UnitKind kind, const h2v_plan *p, uint64_t n, const uint8_t *pairs, uint8_t *accept, uint32_t *status) {
    Unit u{kind, p, (uint32_t)n};
    u.pairs = pairs; u.accept = accept; u.status = status;
    return u;
}
static int fold_pairs_tail(const Unit &u, const uint32_t *er2, const uint32_t *el2, h2v_workspace *w, CallRec &rec, hipStream_t st);
static int agg_chunk(const Unit &u, struct RlcWs *r, h2v_workspace *w, CallRec &rec, hipStream_t st);
// Decompression: ONE launch whose waves (at most one per SIMD) take 64-point units from a queue - all subgroup tests,
// then all square roots (k_g1_decompress_queue).  v: the plan, or a view of it (pair_view); tab: where the MSM window tables
// go (NULL: none are built); blocks_out (h2v_probe_decompress): the grid of the launch.
// (DecBufs: where the points and their two verdict bytes go, and the launch's queue counter - a workspace's own, or the set of
// h2v_check_pairs_multi)
struct DecBufs { uint32_t *pts; uint8_t *valid, *valid_sub; uint32_t *dec_ctr; };
static int launch_decompress(const H2vDevPlan &v, uint32_t n, const uint8_t *src, const uint64_t *off, const uint8_t *ci, const uint8_t *inst,
                             const DecBufs &b, uint32_t *tab, hipStream_t st, uint32_t *blocks_out = nullptr) {
    const uint32_t dec_grid = (n * H2V_SLOTS(v) + 63) / 64, units = 2 * dec_grid, max_blocks = (uint32_t)(msm_n_simd() / 4.0);
    const uint32_t blocks = (units + 3) / 4 < max_blocks ? (units + 3) / 4 : max_blocks;
    if (blocks_out) *blocks_out = blocks;
    HIPCHK(hipMemsetAsync(b.dec_ctr, 0, 4, st));
    hipLaunchKernelGGL(k_g1_decompress_queue, dim3(blocks), dim3(256), 0, st, v, n, src, off, ci, inst, b.pts, b.valid, tab, b.valid_sub, b.dec_ctr, dec_grid);
    return H2V_OK;
}
static int launch_decompress(const H2vDevPlan &v, uint32_t n, const uint8_t *src, const uint64_t *off, const uint8_t *ci, const uint8_t *inst,
                             h2v_workspace *w, uint32_t *tab, hipStream_t st, uint32_t *blocks_out = nullptr) {
    return launch_decompress(v, n, src, off, ci, inst, DecBufs{w->pts, w->valid, w->valid_sub, w->dec_ctr}, tab, st, blocks_out);
}
static int run_pipeline(const Unit &u, h2v_workspace *w, hipStream_t st) {
    const H2vDevPlan &d = u.p->d;
    const uint32_t n = u.n;
    const bool fold = u.kind == UnitKind::FOLD_RLC, mixed = u.kind == UnitKind::MIXED_SUB, prepare = u.kind == UnitKind::PREPARE;
    LaunchOptsScope opts(w);
    const uint32_t slots = H2V_SLOTS(d);
    uint32_t *trace = u.trace ? w->trace : nullptr;
    // H2V_DEBUG_SYNC: after each stage, say which kernel was launched and wait for the whole device, so that a fault is
    // reported at the stage that caused it
    static const bool dbg = getenv("H2V_DEBUG_SYNC") != nullptr;
    auto stage_done = [&](const char *kernel) -> int {
        if (!dbg) return H2V_OK;
        fprintf(stderr, "[h2v] launching %s (n=%u)\n", kernel, n); fflush(stderr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        return H2V_OK;
    };
    // A caller that keeps >= 6 batches in flight (h2v_workspace_hint_in_flight) gets the whole pipeline on ITS stream: the
    // other batches fill the chip, and one stream per batch keeps many batches within the 16 hardware queues (three
    // streams per batch collide from the sixth batch on).  Measured, 40 steps of simple_mul x 4096: three streams 5 / 8 / 11
    // in flight 4.46 / 4.66 / 4.75 ms per step, one stream 4.80 / 4.39 / 4.50.  H2V_OPT_STREAMS forces the choice.
    const bool one_stream = w->one_stream_mode >= 0 ? w->one_stream_mode == 1 : w->in_flight_hint >= 6;
    // one_stream_mode 2 (lanes): the pipeline on the stream it is given, only the decompression beside it on a side stream
    const bool two_stream = w->one_stream_mode == 2;
    if (!one_stream)
        if (int rcs = ws_streams(w, !two_stream, true)) return rcs;
    hipStream_t pm = (one_stream || two_stream) ? st : w->pmain, ps = one_stream ? st : w->pside;
    CallRec &rec = rec_new(w, fold ? h2v_workspace::RLC : (prepare || mixed) ? h2v_workspace::PREPARE : h2v_workspace::VERIFY);
    // fold (H2V_RLC_FOLD_PAIRS): the record's events carry run_rlc's layout - [0]/[1] around the decompression, [2]/[3] around the
    // combiner, the rest recorded by pairs_rlc_core - and the pipeline's own markers go to a set of the workspace that nobody reads
    hipEvent_t *ev = rec.ev;
    if (fold) {
        for (hipEvent_t &e : w->ev_pipe) if (int rce = lazy_event(w->mem, e, hipEventDefault)) return rce;
        ev = w->ev_pipe;
    }
    HIPCHK(hipEventRecord(w->ev_fork, st));
    HIPCHK(hipStreamWaitEvent(pm, w->ev_fork, 0));
    HIPCHK(hipStreamWaitEvent(ps, w->ev_fork, 0));
    HIPCHK(hipEventRecord(ev[2], ps));
    if (fold) HIPCHK(hipEventRecord(rec.ev[0], ps));
    if (int rcl = launch_decompress(d, n, u.proofs, u.off, u.ci, u.inst, w, w->pt_tab, ps)) return rcl;
    HIPCHK(hipEventRecord(ev[3], ps));
    if (fold) HIPCHK(hipEventRecord(rec.ev[1], ps));
    HIPCHK(hipEventRecord(w->ev_join, ps));
    // The MSM's hold: it waits for a few more packets on the side stream than its inputs need (a wait, two timed markers, the
    // marker it waits for).  The MSM wants every SIMD to itself, and it is faster for the small delay: measured with the
    // default simple_mul x 4096 run, five runs each, 1.257 M proofs/s with the hold, 1.248 M with the marker and the wait
    // alone, 1.241 M without any.
    HIPCHK(hipStreamWaitEvent(ps, w->ev_fork, 0));
    HIPCHK(hipEventRecord(ev[10], ps));
    HIPCHK(hipEventRecord(ev[11], ps));
    HIPCHK(hipEventRecord(w->ev_hold, ps));
    if (int rcd = stage_done("k_g1_decompress_queue")) return rcd;
    HIPCHK(hipEventRecord(ev[0], pm));
    if (fold) HIPCHK(hipEventRecord(rec.ev[2], pm));
    if (int rcv = launch_vm(d, n, w->stride, u.proofs, u.off, u.inst, u.ci, w->regs, w->scalars, w->status, trace, pm)) return rcv;
    HIPCHK(hipEventRecord(ev[1], pm));
    if (fold) HIPCHK(hipEventRecord(rec.ev[3], pm));
    if (int rcd = stage_done("k_transcript_combiner")) return rcd;
    HIPCHK(hipStreamWaitEvent(pm, w->ev_join, 0));
    HIPCHK(hipStreamWaitEvent(pm, w->ev_hold, 0));
    HIPCHK(hipEventRecord(ev[4], pm));
    const SegBuf seg = {w->msm_parts, w->shape.segs};   // (NULL for workspaces of plans whose sums are all <= 64 terms)
    const MsmModel mm = msm_model();
    const MsmShape single = msm_ladder_shape(mm, d.ivc ? d.n_terms : d.n_main_terms, n, 0.0, true, d.ivc ? 0u : seg.room());
    const MsmSplit split = w->er_fix && d.fix_tab && !d.ivc ? msm_split_shape(mm, MsmSplitTerms{d.n_var, d.n_fix, d.n_main_terms}, n, single, w->in_flight_hint, seg.room())
                                                            : MsmSplit{false, {}, {}, 0};
    if (split.on) {
        // per-proof terms as ladders on the main stream; the VK-base terms beside them on the side stream (free since
        // the square roots finished), which first waits for the combiner's scalars; a one-lane-per-proof kernel adds
        // the two sums
        const H2vMsmArgs mv = msm_args(d, 0, d.n_var, d.n_terms, 0, slots, w->er, w->pt_tab);
        const H2vMsmArgs mf = msm_fixed_args(d, d.n_terms, d.n_var, w->er_fix, w->pt_tab, split.k);
        HIPCHK(hipStreamWaitEvent(ps, ev[1], 0));
        HIPCHK(hipEventRecord(ev[7], ps));
        launch_msm_fixed(d, mf, n, split.fix.bs, w->scalars, w->pts, ps);
        HIPCHK(hipEventRecord(ev[8], ps));
        HIPCHK(hipEventRecord(w->ev_fix, ps));
        if (ps == pm) HIPCHK(hipEventRecord(ev[4], pm));   // (one stream: the ladder launch starts behind the fixed-base one)
        uint32_t var_code;
        if (msm_terms_per_lane(mm, w->in_flight_hint) > 1) var_code = launch_msm_range(d, mv, n, w->scalars, w->pts, nullptr, pm, w->in_flight_hint, seg);   // (several terms per lane)
        else var_code = launch_msm_ladders(d, mv, n, split.var, w->scalars, w->pts, nullptr, pm, seg);
        if (!var_code) return fail(H2V_E_LIMIT, "internal: no MSM launch shape for the per-proof terms");
        HIPCHK(hipEventRecord(ev[9], pm));
        rec.var_lpt = (uint8_t)var_code;
        HIPCHK(hipStreamWaitEvent(pm, w->ev_fix, 0));
        hipLaunchKernelGGL(k_g1_sum_pairs, dim3((n + 63) / 64), dim3(64), 0, pm, n, w->er, w->er_fix);
        rec.lpt = 3;
    } else {
        rec.lpt = (uint8_t)launch_msm(d, n, w->scalars, w->pts, w->pt_tab, w->er, w->accl, w->accr, pm, w->in_flight_hint, seg);
        if (!rec.lpt) return fail(H2V_E_LIMIT, "internal: no MSM launch shape for this plan");
    }
    if (int rcd = stage_done("k_g1_msm")) return rcd;
    const uint32_t *er_in = w->er, *el_in = nullptr;
    if (d.ivc) {   // (timed with the MSM: the challenge hash and one more pass of the same kernel)
        const IvcBufs ib = {w->accl, w->accr, w->fold_pts, w->fold_scal, w->el2, w->er2};
        launch_ivc_fold(d, n, w->pts, w->er, ib, w->msm_tab, pm);
        er_in = ib.er2; el_in = ib.el2;
        if (int rcd = stage_done("k_ivc_challenge + fold MSM")) return rcd;
    }
    HIPCHK(hipEventRecord(ev[5], pm));
    if (fold) {
        if (int rcf = fold_pairs_tail(u, er_in, el_in, w, rec, pm)) return rcf;
    } else if (mixed)
        hipLaunchKernelGGL(k_mixed_pairs, dim3((n + 63) / 64), dim3(64), 0, pm, d, n, w->pts, w->valid, w->valid_sub, er_in, el_in, (const uint32_t *)w->status, u.pos, u.pool.pool,
                           u.pool.good, u.pool.status);
    else if (prepare)   // (rec.pair stays 0: h2v_workspace_timings reports pairing_ms = 0 for the call)
        hipLaunchKernelGGL(k_prepare_export, dim3((n + 63) / 64), dim3(64), 0, pm, d, n, w->pts, w->valid, w->valid_sub, er_in, el_in, w->status, (uint32_t *)u.pairs_out);
    else
        rec.pair = (uint8_t)launch_pairing(d, n, w->pts, w->valid, w->valid_sub, er_in, el_in, w->status, u.accept, nullptr, pm, w->in_flight_hint);
    HIPCHK(hipEventRecord(ev[6], pm));
    HIPCHK(hipEventRecord(w->ev_done, pm));
    HIPCHK(hipStreamWaitEvent(st, w->ev_done, 0));
    if (int rcd = stage_done(mixed ? "k_mixed_pairs" : prepare ? "k_prepare_export" : "k_pairing")) return rcd;
    HIPCHK(hipGetLastError());
    if (u.status) HIPCHK(hipMemcpyAsync(u.status, w->status, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return H2V_OK;
}

// Pair check: n records of 96 bytes compress(L) || compress(R) are decoded as two-slot "proofs" of a view of the plan (its
// line tables of s_g2 and G2, proof_len 96, slots at bytes 0 and 48) by the pipeline's decompression launch - flags, canonical
// x, on the curve, in G1, infinity allowed - into the workspace's point buffers; R goes to Jacobian form (k_pairs_to_jac) and
// the production pairing launcher checks e(L, s_g2) == e(R, G2).  Everything on `st`.  Events as run_pipeline's:
// [2]/[3] around the decompression, [4]/[5] around the conversion, [5]/[6] around the pairing.
static int pair_view_ensure(h2v_workspace *w) {
    if (w->pair_off) return H2V_OK;
    std::vector<uint64_t> off(w->cap + 1);
    for (uint64_t i = 0; i <= w->cap; i++) off[i] = 96 * i;
    const uint32_t slot_off[2] = {0, 48};
    const auto T = wslayout::pair_view(w->cap);
    if (!w->mem.alloc(w->pair_pts, T.row[wslayout::V_PTS]) || !w->mem.alloc(w->pair_off, T.row[wslayout::V_OFF]) ||
        hipMemcpy(w->pair_pts, slot_off, 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(w->pair_off, off.data(), off.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
        w->mem.drop(w->pair_off); w->mem.drop(w->pair_pts);
        return fail(H2V_E_DEVICE, "allocation of the pair-check buffers failed");
    }
    return H2V_OK;
}
// the two-slot view of plan d on a workspace that has been through pair_view_ensure
static H2vDevPlan pair_view(const H2vDevPlan &d, const h2v_workspace *w) {
    H2vDevPlan v = d;
    v.proof_len = 96; v.n_points = 2; v.n_ci = 0; v.n_pi = 0; v.ivc = 0; v.pi_point = 0; v.points = w->pair_pts;
    return v;
}
static int run_check(const Unit &u, h2v_workspace *w, hipStream_t st) {
    const uint32_t n = u.n;
    LaunchOptsScope opts(w);
    if (int rc = pair_view_ensure(w)) return rc;
    const H2vDevPlan v = pair_view(u.p->d, w);
    CallRec &rec = rec_new(w, h2v_workspace::CHECK);
    hipEvent_t *ev = rec.ev;
    for (int q : {0, 1, 2}) HIPCHK(hipEventRecord(ev[q], st));
    HIPCHK(hipMemsetAsync(w->status, 0, (size_t)n * 4, st));
    if (int rc = launch_decompress(v, n, u.pairs, w->pair_off, nullptr, nullptr, w, nullptr, st)) return rc;
    HIPCHK(hipEventRecord(ev[3], st));
    HIPCHK(hipEventRecord(ev[4], st));
    hipLaunchKernelGGL(k_pairs_to_jac, dim3((n + 63) / 64), dim3(64), 0, st, n, (const uint32_t *)w->pts, w->er, (const uint32_t *)nullptr);
    HIPCHK(hipEventRecord(ev[5], st));
    rec.pair = (uint8_t)launch_pairing(v, n, w->pts, w->valid, w->valid_sub, w->er, nullptr, w->status, u.accept, nullptr, st, w->in_flight_hint);
    HIPCHK(hipEventRecord(ev[6], st));
    HIPCHK(hipGetLastError());
    if (u.status) HIPCHK(hipMemcpyAsync(u.status, w->status, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return H2V_OK;
}

static int run_rlc(const Unit &u, h2v_workspace *w, hipStream_t st);
static int run_pairs_rlc(const Unit &u, h2v_workspace *w, hipStream_t st);
static int run_mixed_tail(const Unit &u, h2v_workspace *w, hipStream_t st);
static int run_mixed_terms(const Unit &u, h2v_workspace *w, hipStream_t st);
static int run_mixed_fold_tail(const Unit &u, h2v_workspace *w, hipStream_t st);
static int run_mixed_group(const Unit &u, h2v_workspace *w, hipStream_t st);
static int run_across_tail(const Unit &u, h2v_workspace *w, hipStream_t st);
// ROUTING of RLC calls (round 4).  The batch-accept mode pays for every batch whose check fails: with 1 % rejecting proofs
// nearly half of the groups of 64 fail, and the call costs 1.3 x the per-proof mode it falls back to.  A workspace therefore
// keeps a running estimate of the rate of FAILING GROUPS among the groups its RLC calls have seen - cumulative device
// counters written by the batch / group checks (or, for a routed call, by k_rlc_count_groups from the status words), mirrored
// into pinned host memory behind every chunk and read without synchronisation at the head of the next call - and sends a
// call straight to the per-proof kernels while that rate is above 0.10 (back to the batch check below 0.05).  Break-even,
// measured (simple_mul x 4096, sixteen calls in flight, ms per call): honest 1.37; one failing group (1 reject) 2.74; 17 % of the
// groups failing (0.3 % rejects) 3.72; the per-proof mode 3.25 whatever it meets: about 2.6 + 6.4 x rate, equal at a rate of 0.1.
// Same accept[] either way; fell_back / h2v_workspace_rlc_result report which path ran.  H2V_OPT_RLC_ROUTE = -1: never route.
// (also the records' verdict words: RLC calls are made on a workspace that has been through here, lanes' chunks excepted - they
// report into their parent's record)
static int rlc_stats_ensure(h2v_workspace *w) {
    if (w->rlc_stats) return H2V_OK;
    const auto T = wslayout::rlc_stats();
    if (!w->mem.alloc(w->rec_fail, T.row[wslayout::S_REC_FAIL]) || !w->mem.alloc(w->rlc_stats, T.row[wslayout::S_RLC_STATS]) ||
        !w->mem.alloc_pinned(w->h_rlc_stats, T.row[wslayout::S_H_RLC_STATS]))
        return fail(H2V_E_DEVICE, "allocation of the routing counters failed");
    w->h_rlc_stats[0] = w->h_rlc_stats[1] = 0;
    return H2V_OK;
}
static bool rlc_route(h2v_workspace *w) {
    if (w->opt[H2V_OPT_RLC_ROUTE] < 0 || !w->h_rlc_stats) return false;
    const volatile uint32_t *h = w->h_rlc_stats;
    const uint32_t g = h[0], f = h[1];
    const uint32_t dg = g - w->seen_groups, df = f - w->seen_failed;
    if (dg) {
        const float rate = df >= dg ? 1.0f : (float)df / (float)dg;
        w->fail_rate = 0.75f * w->fail_rate + 0.25f * rate;
        w->seen_groups = g; w->seen_failed = f;
    }
    w->routed = w->routed ? w->fail_rate > 0.05f : w->fail_rate > 0.10f;
    return w->routed;
}
// the counters to their pinned mirror, behind an RLC or routed unit on `st`
static int rlc_stats_mirror(h2v_workspace *w, hipStream_t st) {
    if (hipMemcpyAsync(w->h_rlc_stats, w->rlc_stats, 8, hipMemcpyDeviceToHost, st) != hipSuccess) return fail(H2V_E_DEVICE, "routing counters: copy failed");
    return H2V_OK;
}
// a routed chunk / call: the per-proof pipeline (its record: a routed RLC call), then the counters (a lane's: its parent's)
// from its status words
static int run_routed(const Unit &u, h2v_workspace *w, hipStream_t st) {
    int rc = run_pipeline(u, w, st);
    if (rc) return rc;
    rec_last(w).kind = h2v_workspace::RLC;
    rec_last(w).routed = true;
    hipLaunchKernelGGL(k_rlc_count_groups, dim3(((u.n + 63) / 64 + 63) / 64), dim3(64), 0, st, u.n, w->status, w->rlc_stats_ptr ? w->rlc_stats_ptr : w->rlc_stats);
    HIPCHK(hipGetLastError());
    return H2V_OK;
}
static int run_unit(const Unit &u, h2v_workspace *w, hipStream_t st) {
    switch (u.kind) {
    case UnitKind::CHECK: return run_check(u, w, st);
    case UnitKind::RLC: return run_rlc(u, w, st);
    case UnitKind::PAIR_RLC: return run_pairs_rlc(u, w, st);
    case UnitKind::ROUTED: return run_routed(u, w, st);
    case UnitKind::MIXED_TAIL: case UnitKind::MIXED_TAIL_RLC: return run_mixed_tail(u, w, st);
    case UnitKind::MIXED_SUB_TERMS: return run_mixed_terms(u, w, st);
    case UnitKind::MIXED_FOLD_TAIL: return run_mixed_fold_tail(u, w, st);
    case UnitKind::MIXED_GROUP: return run_mixed_group(u, w, st);
    case UnitKind::MIXED_ACROSS_TAIL: return run_across_tail(u, w, st);
    case UnitKind::VERIFY: case UnitKind::PREPARE: case UnitKind::FOLD_RLC: case UnitKind::MIXED_SUB: break;
    }
    return run_pipeline(u, w, st);
}
// A call on a laned workspace: chunks of at most w->chunk proofs, round robin through the lanes (continuing where the
// previous call stopped).  Chunk c runs on its lane's own stream(s) behind everything the caller had enqueued on `st`
// before the call and behind the lane's earlier chunks.  Nothing else orders the chunks: the kernels of neighbouring
// chunks drift apart by themselves (a decompression launch wants every SIMD, so the second one queues behind the first),
// and an explicit stagger - chunk c waiting for phase 1 of chunk c - 1 - measured 10-20 % slower.  Batch checks: every chunk is
// its own.
// How many lanes a call of n proofs cycles through, and (per-proof mode) the streams of a chunk.  Chunks that give the MSM
// at most half a wave per SIMD are chains of lone waves - latency, not issue slots - and want as many of them in flight
// as there are streams: every lane, each chunk on its lane's stream alone.  Larger chunks: H2V_PER_PROOF_LANES lanes, the
// decompression on a side stream.  Measured (ms per batch; 8 lanes two streams each -> 16 lanes one stream each): secp256k1
// shape x 64 0.87 -> 0.57, x 128 1.12 -> 0.74; sha256 shape x 128 0.94 -> 0.74, x 256 1.29 -> 0.90, x 512 1.45 -> 1.24, secp256k1
// x 512 1.51 -> 1.34, simple_mul x 1024 1.48 -> 1.23; simple_mul x 2048 and sha256 x 1024: the same either way (2.16 / 2.18).
// An explicit lane count (h2v_workspace_create_lanes) is kept; H2V_OPT_STREAMS forces the streams.
static uint32_t laned_depth(const h2v_workspace *w, uint64_t n, bool rlc, int *stream_mode) {
    if (stream_mode) *stream_mode = 1;
    if (rlc) return w->n_lanes;
    const uint64_t m = n < w->chunk ? n : w->chunk;
    const bool small = (double)m * w->shape.terms / 64.0 <= msm_n_simd() / 2.0;
    if (stream_mode) {
        *stream_mode = w->one_stream_mode >= 0 ? w->one_stream_mode : small ? 1 : 2;
    }
    return (small || w->lanes_per_proof >= w->n_lanes) ? w->n_lanes : w->lanes_per_proof;
}
// What the chunks' launch shapes may assume about the chip: with deferred joins (and the host-buffer stream of batches)
// consecutive calls overlap and every lane is busy; a call that waits for its own chunks has only THOSE in flight - one
// 4096-proof chunk on a laned workspace is a lone batch (with the full-chip shapes it took 11.6 ms instead of 5.8).
// lanes_stay_full: the caller knows that the lanes are full whatever this call brings; own: what this call alone puts in flight.
static uint32_t call_hint(const h2v_workspace *w, bool lanes_stay_full, uint32_t own) {
    return w->hint_given ? w->in_flight_hint : (w->defer_joins || lanes_stay_full) ? w->n_lanes : own;
}
static uint32_t n_chunks(uint32_t n, uint32_t chunk) { return (n + chunk - 1) / chunk; }
// the record of a call of n proofs on a laned workspace, cut into `chunk`s that cycle through L lanes from where the previous
// call stopped
static CallRec &rec_laned(h2v_workspace *w, h2v_workspace::Kind kind, uint32_t L, uint32_t n, uint32_t chunk) {
    CallRec &rec = rec_new(w, kind);
    rec.first = (uint32_t)(w->next_lane % L); rec.mod = L; rec.chunks = n_chunks(n, chunk);
    for (uint32_t l = 0; l < w->n_lanes; l++) rec.start[l] = w->lane[l] ? w->lane[l]->calls : 0;   // (every chunk takes one record on its lane)
    return rec;
}
// One unit on lane l.  hint: what its launch shapes may assume (call_hint); stream_mode: the streams of a pipeline (laned_depth) -
// a routed unit runs on the lane's stream alone, and a batch check or a pair check keeps the lane's streams as they are.  Behind
// an RLC or routed unit the workspace's failing-group counters go to their mirror.
struct LaneSetup { uint32_t hint; int stream_mode; };
static int run_on_lane(h2v_workspace *w, uint32_t l, const Unit &u, const LaneSetup &s) {
    h2v_workspace *lw = w->lane[l];
    const bool counted = (u.kind == UnitKind::RLC || u.kind == UnitKind::ROUTED) && !u.agg_parts;   // (an aggregate call moves no estimate)
    lw->in_flight_hint = s.hint;
    lw->opt[H2V_OPT_RLC_GROUP_STAGE] = w->opt[H2V_OPT_RLC_GROUP_STAGE];
    if (counted) lw->rlc_stats_ptr = w->rlc_stats;
    if (u.kind == UnitKind::ROUTED) lw->one_stream_mode = 1;
    else if (u.kind == UnitKind::VERIFY || u.kind == UnitKind::PREPARE || u.kind == UnitKind::FOLD_RLC || u.kind == UnitKind::MIXED_SUB || u.kind == UnitKind::MIXED_SUB_TERMS ||
             u.kind == UnitKind::MIXED_GROUP)
        lw->one_stream_mode = s.stream_mode;
    int rc = run_unit(u, lw, w->lane_st[l]);
    if (rc == H2V_OK && counted) rc = rlc_stats_mirror(w, w->lane_st[l]);
    return rc;
}
// the end of lane l's most recent chunk, for the joins
static int lane_done(h2v_workspace *w, uint32_t l) {
    HIPCHK(hipEventRecord(w->lane_ev[l], w->lane_st[l]));
    w->lane_busy[l] = true;
    return H2V_OK;
}
// THE chunk loop: unit u in `chunk`s round robin through L lanes, each behind the caller's w->ev_fork.  before(lane, stream) runs
// before a chunk is enqueued on its lane (the mixed tail: its waits for the sub-batches' lanes).  An error of a chunk comes back
// drained: earlier chunks of this call and of calls before it are in flight on other lanes.
template <class Before> static int run_chunks(h2v_workspace *w, const Unit &u, uint32_t L, uint32_t chunk, const LaneSetup &s, Before &&before) {
    for (uint32_t c = 0, nch = n_chunks(u.n, chunk); c < nch; c++) {
        const uint32_t l = (uint32_t)(w->next_lane++ % L);
        if (int rc = ensure_lane(w, l)) return rc;
        HIPCHK(hipStreamWaitEvent(w->lane_st[l], w->ev_fork, 0));
        if (int rc = before(l, w->lane_st[l])) return rc;
        const uint32_t lo = c * chunk;
        Unit cu = u.slice(lo, (u.n - lo) < chunk ? (u.n - lo) : chunk);
        cu.seed[7] ^= 0x9e3779b9u * (c + 1);      // (a chunk is its own batch check: its own coefficients)
        cu.seed_xor7 ^= 0x9e3779b9u * (c + 1);    // (the same tweak for a derived seed, which is read on the device)
        cu.part = c;
        if (int rc = run_on_lane(w, l, cu, s)) return drain_after_error(w, rc);
        if (int rc = lane_done(w, l)) return rc;
    }
    return H2V_OK;
}
// when `st` waits for the lanes of a call: as the workspace defers its joins or not, now whatever it defers, or not at all (the
// streamed host batches: their downloads wait for their own lanes)
enum class Join { AS_DEFERRED, NOW, NEVER };
static int co_flush(h2v_workspace *w);
static int run_laned(Unit u, h2v_workspace *w, hipStream_t st, Join join) {
    if (int rcf = co_flush(w)) return rcf;          // (calls start in submission order: an open group of coalesced calls first)
    int stream_mode = 1;
    const uint32_t n = u.n;
    const uint32_t L = laned_depth(w, n, u.kind == UnitKind::RLC || u.kind == UnitKind::PAIR_RLC, &stream_mode);
    // A per-proof call that would leave lanes empty at the workspace's chunk size is cut finer, one chunk per lane (in 512s,
    // not below 2048: there the chains' latency costs more than the extra lanes win).  One call on 20 480 simple_mul proofs,
    // eight lanes: chunks of 4096 24.0 ms, 2560 22.5 ms, 2048 27.7 ms.  (RLC mode: every chunk is a batch check of its own and
    // 4096 measured best - 45 056 proofs in 4096s 19.3 ms, in 2816s 20.6 ms.)
    uint32_t chunk = w->chunk;
    // (only for a call that waits for its own chunks: with deferred joins or streamed host batches the NEXT call fills the lanes,
    //  and whole chunks keep the full-chip launch shapes - a stream of 16 384-proof calls: 15.9 ms per call cut in 2048s, ~13 in 4096s)
    if (!u.batch_check() && !w->defer_joins && join != Join::NEVER && n > chunk && (uint64_t)n < (uint64_t)L * chunk) {
        const uint32_t c2 = (uint32_t)(((n + L - 1) / L + 511) / 512 * 512);
        if (c2 >= default_chunk(wslayout::shape_of(u.p->d, false)) / 2 && c2 < chunk) chunk = c2;       // (simple_mul: 2048; T = 60: 512)
    }
    const uint32_t nch = n_chunks(n, chunk);
    CallRec &rec = rec_laned(w, u.batch_check() ? h2v_workspace::RLC : u.kind == UnitKind::CHECK ? h2v_workspace::CHECK : u.kind == UnitKind::PREPARE ? h2v_workspace::PREPARE : h2v_workspace::VERIFY,
                             L, n, chunk);
    if (u.batch_check()) {
        // the chunks report into this record's word.  RLC over proofs: routed - "a batch check failed" = the per-proof kernels
        // produce accept[]; over pairs (given or folded): never routed, and the failing-group estimate stays where it is
        if (int rcs = rlc_stats_ensure(w)) return rcs;
        if (u.kind == UnitKind::RLC && !u.agg_parts && (rec.routed = u.route)) u.kind = UnitKind::ROUTED;   // (run_call's decision; an aggregate call is never routed)
        rec.agg = u.agg_parts != nullptr;
        HIPCHK(hipMemsetAsync(rec_word(w, rec), rec.routed ? 1 : 0, 4, st));
        u.fail_ctr = rec_word(w, rec);
        u.one_stream_opt = true;
    }
    HIPCHK(hipEventRecord(w->ev_fork, st));
    // (a call that waits for its own chunks has only those in flight; streamed host batches keep every lane busy)
    const LaneSetup setup = {call_hint(w, join == Join::NEVER, nch < L ? nch : L), stream_mode};
    if (int rc = run_chunks(w, u, L, chunk, setup, [](uint32_t, hipStream_t) { return H2V_OK; })) return rc;
    if (join == Join::NEVER) return H2V_OK;
    if (!w->defer_joins || join == Join::NOW) return lanes_join(w, st);
    return H2V_OK;
}
// ---- coalescing of small calls (round 4; VERDICT r3 #6: "let lanes pack units of several small calls of the same plan into one
// launch per kernel").  A device-resident call (per proof, or RLC among RLC calls) of at most HALF a chunk on a laned workspace with deferred joins is not
// launched by itself: its proofs are gathered (h2v_coalesce.hpp, on a lane's stream, behind whatever the caller's stream held at
// the time of the call - so the caller's buffers are read at once, as always) behind those of the calls before it, and the
// pipeline runs ONCE over the group - when the next call would not fit, when a call of another plan or kind arrives, or at
// h2v_workspace_join - after which every call's accept[] / status[] are copied to where the caller wanted them.  That is within
// the contract of deferred joins as it stood (results are the caller's after h2v_workspace_join); what changes is how the work
// is cut: sixteen 64-proof calls are one 1024-proof launch per kernel instead of sixteen chains of lone waves.  Verdicts cannot
// depend on it (a proof's verdict depends on its own bytes; tests/test_gpu_parity.py::test_small_calls_are_coalesced).
// H2V_OPT_COALESCE = -1 on the workspace switches it off.
struct Coalesce {
    Owner mem;
    uint8_t *proofs = nullptr, *inst = nullptr, *ci = nullptr, *accept = nullptr;
    // one allocation: the group's verdict word (RLC: failed batch checks; 8 bytes) and behind it off[0 .. cap], so that the one
    // memset that opens a group zeroes both
    uint32_t *fail = nullptr;
    uint64_t *off = nullptr;
    uint32_t *status = nullptr;
    size_t cap_proof_bytes = 0, cap_inst = 0;
    uint32_t cap = 0;                    // proofs
    const h2v_plan *plan = nullptr;      // of the open group
    uint64_t plan_gen = 0;
    uint32_t count = 0;
    bool rlc = false;                    // the open group's mode: per proof, or ONE batch check over the whole group
    uint32_t seed[8] = {};               // (RLC: the first call's - one fresh seed makes every coefficient unpredictable)
    struct Part { uint8_t *accept; uint32_t *status; uint32_t base, n; uint64_t call; };
    std::vector<Part> parts;
};
static void co_release(h2v_workspace *w) {
    for (auto &c : w->co) {
        if (!c) continue;
        c->mem.release();
        delete c;
        c = nullptr;
    }
    w->co_open.clear();
}
// the staging buffers of lane l for groups of plan p (grown when a plan with longer proofs / more public inputs comes along)
static int co_ensure(h2v_workspace *w, uint32_t l, const h2v_plan *p) {
    if (!w->co[l]) w->co[l] = new Coalesce();
    Coalesce &c = *w->co[l];
    const uint32_t cap = w->chunk;
    const size_t need_p = wslayout::co_proof_bytes(cap, p->d.proof_len), need_i = wslayout::co_inst_bytes(cap, p->d.n_pi);
    if (c.cap == cap && c.cap_proof_bytes >= need_p && c.cap_inst >= need_i) return H2V_OK;
    HIPCHK(hipStreamSynchronize(w->lane_st[l]));              // (an earlier group may still be running out of the old buffers)
    c.mem.release();
    c.off = nullptr; c.cap = 0;
    const size_t bp = need_p > c.cap_proof_bytes ? need_p : c.cap_proof_bytes, bi = need_i > c.cap_inst ? need_i : c.cap_inst;
    const auto T = wslayout::coalesce(cap, bp, bi);
    const bool ok = c.mem.alloc(c.proofs, T.row[wslayout::C_PROOFS]) && c.mem.alloc(c.inst, T.row[wslayout::C_INST]) && c.mem.alloc(c.ci, T.row[wslayout::C_CI]) &&
                    c.mem.alloc(c.accept, T.row[wslayout::C_ACCEPT]) && c.mem.alloc(c.fail, T.row[wslayout::C_FAIL]) && c.mem.alloc(c.status, T.row[wslayout::C_STATUS]);
    if (!ok) return fail(H2V_E_DEVICE, "hipMalloc(coalescing buffers) failed");
    c.off = (uint64_t *)c.fail + 1;
    c.cap = cap; c.cap_proof_bytes = bp; c.cap_inst = bi;
    return H2V_OK;
}
// runs every open group, oldest first
static int co_flush_lane(h2v_workspace *w, uint32_t l);
static int co_flush(h2v_workspace *w) {
    while (!w->co_open.empty())
        if (int rc = co_flush_lane(w, w->co_open.front())) return rc;
    return H2V_OK;
}
// runs the open group of lane l: ONE pass of the pipeline over everything gathered so far, then every call's verdicts to the caller's buffers
static int co_flush_lane(h2v_workspace *w, uint32_t l) {
    for (size_t k = 0; k < w->co_open.size(); k++)
        if (w->co_open[k] == l) { w->co_open.erase(w->co_open.begin() + (long)k); break; }
    Coalesce &c = *w->co[l];
    if (c.count == 0) return H2V_OK;
    h2v_workspace *lw = w->lane[l];
    hipStream_t ls = w->lane_st[l];
    int stream_mode = 1;
    (void)laned_depth(w, c.count, false, &stream_mode);
    const h2v_plan *p = c.plan;
    const h2v_batch group = {c.count, c.proofs, c.off, p->d.n_pi ? c.inst : nullptr, p->d.n_ci ? c.ci : nullptr};
    Unit u = unit_of_batch(c.rlc ? UnitKind::RLC : UnitKind::VERIFY, p, &group, c.accept, c.status);
    int rc = H2V_OK;
    bool routed = false;
    if (c.rlc) {
        // one batch check over the group (as a chunk of run_laned), reporting into the group's own verdict word (zeroed when
        // the group was opened); copied below into the calls' records
        if ((rc = rlc_stats_ensure(w)) == H2V_OK && (routed = rlc_route(w))) u.kind = UnitKind::ROUTED;
        memcpy(u.seed, c.seed, sizeof u.seed);
        u.fail_ctr = c.fail;
        u.one_stream_opt = true;
    }
    lw->one_stream_mode = stream_mode;      // (a group's batch check too: it runs with the streams of a per-proof group of its size)
    // (groups are gathered with deferred joins: the next calls keep every lane busy)
    if (rc == H2V_OK) rc = run_on_lane(w, l, u, {call_hint(w, true, 0), stream_mode});
    for (const Coalesce::Part &q : c.parts) {
        if (rc) break;
        if (hipMemcpyAsync(q.accept, c.accept + q.base, q.n, hipMemcpyDeviceToDevice, ls) != hipSuccess ||
            (q.status && hipMemcpyAsync(q.status, c.status + q.base, (size_t)q.n * 4, hipMemcpyDeviceToDevice, ls) != hipSuccess))
            rc = fail(H2V_E_DEVICE, "coalesced calls: copying the verdicts out failed");
        // the call's record, unless a later call has taken it: its group ran as this lane's most recent call; its share of that
        // launch; the group's verdict (routed: "a batch check failed" = the per-proof kernels produce accept[])
        CallRec *r = rec_at(w, q.call);
        if (!r || rc) continue;
        if (c.rlc && (routed ? hipMemsetAsync(rec_word(w, *r), 1, 4, ls) : hipMemcpyAsync(rec_word(w, *r), c.fail, 4, hipMemcpyDeviceToDevice, ls)) != hipSuccess)
            rc = fail(H2V_E_DEVICE, "coalesced calls: copying the batch verdict out failed");
        r->ran = true; r->share = (float)q.n / (float)c.count; r->routed = routed;
        r->first = l; r->mod = w->n_lanes; r->chunks = 1; r->start[l] = lw->calls - 1;
    }
    c.parts.clear();
    c.count = 0;
    c.plan = nullptr;
    if (rc) return drain_after_error(w, rc);
    return lane_done(w, l);
}
static bool co_wanted(const h2v_workspace *w, uint64_t n) {
    return w->n_lanes && w->defer_joins && w->opt[H2V_OPT_COALESCE] >= 0 && n * 2 <= w->chunk && !w->pending;
}
// one small call (VERIFY or RLC): gathered into the open group (opening one, or running the open one first when this call does not fit it)
static int coalesce_call(const Unit &u, h2v_workspace *w, hipStream_t st) {
    const h2v_plan *p = u.p;
    const uint32_t n = u.n;
    const bool rlc = u.kind == UnitKind::RLC;
    // the open group of this plan and mode (a workspace that serves several plans keeps one group per plan open: calls that
    // alternate between two plans would otherwise run every group at one call)
    int found = -1;
    for (uint32_t q : w->co_open) {
        const Coalesce &o = *w->co[q];
        if (o.plan == p && o.plan_gen == p->gen && o.rlc == rlc) { found = (int)q; break; }
    }
    if (found >= 0 && w->co[found]->count + n > w->co[found]->cap) {
        if (int rcf = co_flush_lane(w, (uint32_t)found)) return rcf;
        found = -1;
    }
    if (found < 0) {
        int sm = 1;
        const uint32_t L = laned_depth(w, w->chunk, false, &sm);
        // at most four groups open, and never as many as there are lanes to put them on (a workspace of three lanes that served
        // five plans opened a group on a lane that still held one: its calls were never run - found by tests/soak.py)
        const size_t max_open = L < 4 ? L : 4;
        while (w->co_open.size() >= max_open)
            if (int rcf = co_flush_lane(w, w->co_open.front())) return rcf;
        uint32_t l = (uint32_t)(w->next_lane++ % L);
        for (uint32_t tries = 0; tries < L; tries++) {          // (a lane whose group is still open is not a place for another)
            bool taken = false;
            for (uint32_t q : w->co_open) taken = taken || q == l;
            if (!taken) break;
            l = (uint32_t)(w->next_lane++ % L);
        }
        int rc = ensure_lane(w, l);
        if (rc) return rc;
        if ((rc = co_ensure(w, l, p))) return rc;
        Coalesce &c = *w->co[l];
        c.plan = p; c.plan_gen = p->gen; c.count = 0; c.parts.clear();
        c.rlc = rlc;
        copy_seed(c.seed, rlc ? u.seed : nullptr);
        HIPCHK(hipMemsetAsync(c.fail, 0, 16, w->lane_st[l]));   // verdict word and off[0] = 0: behind the previous group's flush on this stream
        w->co_open.push_back(l);
        found = (int)l;
    }
    const uint32_t l = (uint32_t)found;
    Coalesce &c = *w->co[l];
    hipStream_t ls = w->lane_st[l];
    HIPCHK(hipEventRecord(w->ev_fork, st));
    HIPCHK(hipStreamWaitEvent(ls, w->ev_fork, 0));
    hipLaunchKernelGGL(k_coalesce_offsets, dim3(1), dim3(256), 0, ls, u.off, n, p->d.proof_len, c.off + c.count);
    hipLaunchKernelGGL(k_coalesce_copy, dim3(n), dim3(256), 0, ls, u.proofs, u.off, c.proofs, c.off + c.count, n);
    HIPCHK(hipGetLastError());
    if (p->d.n_pi) HIPCHK(hipMemcpyAsync(c.inst + (size_t)c.count * p->d.n_pi * 32, u.inst, (size_t)n * p->d.n_pi * 32, hipMemcpyDeviceToDevice, ls));
    if (p->d.n_ci) HIPCHK(hipMemcpyAsync(c.ci + (size_t)c.count * 48, u.ci, (size_t)n * 48, hipMemcpyDeviceToDevice, ls));
    // the call's record: where its group ran is filled in by the flush (co_flush_lane)
    CallRec &rec = rec_new(w, rlc ? h2v_workspace::RLC : h2v_workspace::VERIFY);
    rec.co = true;
    c.parts.push_back({u.accept, u.status, c.count, n, rec.call});
    c.count += n;
    w->lane_busy[l] = true;              // (h2v_workspace_join must look at this lane; its event is recorded by the flush)
    if (c.count >= c.cap) return co_flush_lane(w, l);
    return H2V_OK;
}
// an RLC call on an ORDINARY workspace: the batch check, or - routed - the per-proof pipeline (its record's word: "failed")
static int run_rlc_or_routed(Unit u, h2v_workspace *w, hipStream_t st) {
    int rc;
    if (u.route) u.kind = UnitKind::ROUTED;      // (run_call's decision)
    if ((rc = run_unit(u, w, st))) return rc;
    if (u.kind == UnitKind::ROUTED) HIPCHK(hipMemsetAsync(rec_word(w, rec_last(w)), 1, 4, st));
    return rlc_stats_mirror(w, st);
}
// a call of its own (not gathered into a group) on either form of workspace
// THE entry of every batch-accept call (and of the per-proof calls): the routing decision of an RLC call over proofs, then - a call
// with H2V_RLC_SEED_TRANSCRIPT that is not routed - the digest launches of its derived seed (seed_enqueue: the one place that
// queues them; on `st`, so behind the upload of a host form, and in front of everything the call forks from `st`), then the call.
// The call's record is the next one of `ws` - nothing in between takes one (co_flush takes the lanes', coalesced calls took
// theirs when they were made) -, and its slot of the seed ring is the record's.
static int seed_enqueue(Unit &u, h2v_workspace *ws, hipStream_t st);
static int run_call(Unit u, h2v_workspace *ws, hipStream_t st, Join join = Join::AS_DEFERRED) {
    int rc;
    if (ws->n_lanes && (rc = co_flush(ws))) return rc;      // (calls start in submission order; an open group may move the estimate)
    if (u.kind == UnitKind::RLC && !u.agg_parts) {
        if ((rc = rlc_stats_ensure(ws))) return rc;
        u.route = rlc_route(ws);
    }
    const uint64_t call = ws->calls;
    const bool derive = u.derive && u.batch_check() && !u.route;
    if (derive && (rc = seed_enqueue(u, ws, st))) return rc;
    rc = ws->n_lanes ? run_laned(u, ws, st, join) : (u.kind == UnitKind::RLC && !u.agg_parts) ? run_rlc_or_routed(u, ws, st) : run_unit(u, ws, st);
    if (rc == H2V_OK && derive)
        if (CallRec *r = rec_at(ws, call)) r->derived = true;
    return rc;
}
// The argument rules of a batch with proofs in it
static int batch_args(const h2v_plan *p, const h2v_batch *b) {
    if (!b->proofs || !b->proof_off) return fail(H2V_E_ARG, "null proofs / offsets");
    if (p->d.n_pi && !b->instances) return fail(H2V_E_ARG, "plan has public inputs but instances == NULL");
    if (p->d.n_ci && !b->committed) return fail(H2V_E_ARG, "plan has a committed instance but committed == NULL");
    return H2V_OK;
}
// The temporary workspace of a call that was given none: freed when the entry point returns, which `finish` makes wait for the
// call's stream first (the enqueued kernels use the workspace's buffers).
struct TmpWs {
    h2v_workspace *ws = nullptr;
    ~TmpWs() { if (ws) h2v_workspace_free(ws); }
    int make(const h2v_plan *p, uint64_t n, h2v_workspace *&ws_io) {
        if (ws_io) return H2V_OK;
        if (int rc = ws_create_for(wslayout::shape_of(p->d, false), p->device, n, &ws)) return rc;
        ws_io = ws;
        return H2V_OK;
    }
    int finish(int rc, hipStream_t st) const {
        if (ws && rc == H2V_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(H2V_E_DEVICE, "stream synchronize failed");
        return rc;
    }
};

extern "C" int h2v_verify_batch_device(const h2v_plan *p, const h2v_batch *b, uint8_t *accept, uint32_t *status,
                                       h2v_workspace *ws, void *stream, h2v_timings *timings) {
    if (!p || !b || !accept) return fail(H2V_E_ARG, "null argument");
    if (b->n == 0) return H2V_OK;
    if (int rca = batch_args(p, b)) return rca;
    ALIVE(p); ALIVE(ws);
    HIPCHK(hipSetDevice(p->device));
    TmpWs tmp;
    if (int rct = tmp.make(p, b->n, ws)) return rct;
    if (int rcf = ws_fits(ws, p, b->n, false)) return rcf;
    if (ws->pending) return fail(H2V_E_ARG, "the workspace has a host batch in flight: call h2v_verify_batch_wait first");
    if (int rcn = null_stream_check(ws, stream)) return rcn;
    const Unit u = unit_of_batch(UnitKind::VERIFY, p, b, accept, status);
    if (!timings && co_wanted(ws, b->n)) return coalesce_call(u, ws, (hipStream_t)stream);
    int rc = run_call(u, ws, (hipStream_t)stream, timings ? Join::NOW : Join::AS_DEFERRED);
    if (rc == H2V_OK && timings) {
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        rc = h2v_workspace_timings(ws, 0, timings);
    }
    return tmp.finish(rc, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------- measured launch shapes
// h2v_workspace_tune: instead of trusting the launcher's thresholds (calibrated on five shapes on one chip), MEASURE the
// candidate shapes for THIS plan, batch size and workspace regime once and leave the winner on the workspace.  The batch is
// run repeatedly in the way the workspace will be used - a laned workspace with as many calls in flight as it has lanes for
// that size (deferred joins), an ordinary one call by call - because the shapes interact: the six-lane pairing engine is the
// slowest engine alone and the fastest one in a full pipeline.  Coordinate descent over the two dimensions that matter per
// call (pairing engine, MSM terms per lane): the launcher's own choice first, then each neighbouring engine, then each
// terms-per-lane value with the best engine.  A candidate replaces the incumbent only if it is more than 3 % faster.
// accept[] goes to a scratch buffer: verdicts do not depend on shapes (tests/test_gpu_parity.py).
extern "C" int h2v_workspace_tune(const h2v_plan *p, const h2v_batch *b, h2v_workspace *ws, void *stream, uint32_t flags, h2v_tune_report *rep) {
    if (!p || !b || !ws) return fail(H2V_E_ARG, "null argument");
    ALIVE(p); ALIVE(ws);
    if (flags != 0) return fail(H2V_E_ARG, "flags must be 0 (the per-proof mode is what is tuned)");
    if (b->n == 0 || !b->proofs || !b->proof_off) return fail(H2V_E_ARG, "tuning needs a representative device-resident batch");
    if (int rca = batch_args(p, b)) return rca;
    HIPCHK(hipSetDevice(p->device));
    if (int rcf = ws_fits(ws, p, b->n, false)) return rcf;
    if (ws->pending) return fail(H2V_E_ARG, "the workspace has a host batch in flight: call h2v_verify_batch_wait first");
    hipStream_t st = (hipStream_t)stream;
    const bool laned = ws->n_lanes != 0;
    if (laned && !st) return fail(H2V_E_ARG, "tuning a laned workspace keeps calls in flight: it needs a stream of its own, not the legacy NULL stream");
    const uint32_t n = (uint32_t)b->n;
    const bool co = laned && ws->opt[H2V_OPT_COALESCE] >= 0 && (uint64_t)n * 2 <= ws->chunk;     // (small calls run gathered: that is the regime to measure)
    const uint32_t depth = !laned ? 1u : co ? (ws->chunk / n) * laned_depth(ws, ws->chunk, false, nullptr) : laned_depth(ws, n, false, nullptr);   // (co: a group on every lane)
    const uint32_t m = laned && n > ws->chunk ? ws->chunk : co ? ws->chunk / n * n : n;         // proofs per launch
    const double S = msm_n_simd();
    Owner tmp;                                // of the three below
    uint8_t *acc_tmp = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!tmp.alloc(acc_tmp, n) || !tmp.event(e0, hipEventDefault) || !tmp.event(e1, hipEventDefault)) {
        tmp.release();
        return fail(H2V_E_DEVICE, "tuning: allocation failed");
    }
    const bool saved_defer = ws->defer_joins;
    const int32_t saved_pair = ws->opt[H2V_OPT_PAIRING_ENGINE], saved_tpl = ws->opt[H2V_OPT_MSM_TERMS_PER_LANE];
    int rc = H2V_OK;
    auto set2 = [&](int32_t pairing, int32_t tpl) {
        (void)h2v_workspace_set_option(ws, H2V_OPT_PAIRING_ENGINE, pairing);
        (void)h2v_workspace_set_option(ws, H2V_OPT_MSM_TERMS_PER_LANE, tpl);
    };
    const Unit u = unit_of_batch(UnitKind::VERIFY, p, b, acc_tmp, nullptr);
    auto round_of_calls = [&](uint32_t calls) -> int {
        for (uint32_t k = 0; k < calls; k++) {
            int r = co ? coalesce_call(u, ws, st) : run_call(u, ws, st);
            if (r) return r;
        }
        return laned ? lanes_join(ws, st) : H2V_OK;
    };
    uint32_t n_meas = 0;
    float per_call_ms = 0;                    // (the first measurement's result)
    auto measure = [&](int32_t pairing, int32_t tpl, float *ms) -> int {
        set2(pairing, tpl);
        if (laned) ws->defer_joins = true;
        int r = round_of_calls(depth);                                  // fills the lanes (and creates them)
        if (r) return r;
        // three rounds of the lanes, and at least ~120 ms once the first measurement has told what a call takes: the candidates of a
        // small batch differ by a few per cent of a fraction of a millisecond (secp256k1 shape x 256: the 38 ms measurements of
        // round 4's first tuner picked the narrow engine in one run and the normal one, 13 % faster, in the next)
        uint32_t calls = laned ? 3 * depth : 4;
        if (per_call_ms > 0) {
            const uint32_t want = (uint32_t)(120.0f / per_call_ms) + 1;
            calls = want > calls ? (want < 40 * depth ? want : 40 * depth) : calls;
            if (co) calls = (calls + depth - 1) / depth * depth;     // (whole rounds of full groups)
        }
        if (hipEventRecord(e0, st) != hipSuccess) return fail(H2V_E_DEVICE, "event record failed");
        if ((r = round_of_calls(calls))) return r;
        if (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) return fail(H2V_E_DEVICE, "tuning: the measured calls failed");
        float t = 0;
        if (hipEventElapsedTime(&t, e0, e1) != hipSuccess) return fail(H2V_E_DEVICE, "event timing failed");
        *ms = t / (float)calls;
        if (per_call_ms == 0) per_call_ms = *ms;
        n_meas++;
        return H2V_OK;
    };
    float best_ms = 0, def_ms = 0;
    int32_t best_pair = 0, best_tpl = 0;
    do {
        if ((rc = measure(0, 0, &def_ms))) break;
        if (laned && 120.0f / def_ms > 3.0f * (float)depth && (rc = measure(0, 0, &def_ms))) break;   // (the baseline at the candidates' length)
        best_ms = def_ms;
        const int32_t *eng = nullptr;
        const int n_eng = pairing_tune_candidates(S, m, &eng);
        // (the fastest candidate replaces the launcher's rule when it is 3 % faster than THAT - not each candidate against the best so
        //  far, which favoured whichever engine happened to be measured first)
        float cand_ms = 0;
        int32_t cand = 0;
        for (int k = 0; k < n_eng && !rc; k++) {
            float t;
            if ((rc = measure(eng[k], 0, &t))) break;
            if (cand == 0 || t < cand_ms) { cand_ms = t; cand = eng[k]; }
        }
        if (rc) break;
        if (cand && cand_ms < best_ms * 0.97f) { best_ms = cand_ms; best_pair = cand; }
        const bool ladders_share = !p->d.ivc && (double)m * p->d.n_main_terms / 64.0 >= S / 8.0;   // (k_g1_msm_multi's own preconditions)
        float cand_t_ms = 0;
        int32_t cand_tpl = 0;
        for (int32_t tpl = 2; tpl <= 4 && ladders_share && !rc; tpl++) {
            float t;
            if ((rc = measure(best_pair, tpl, &t))) break;
            if (cand_tpl == 0 || t < cand_t_ms) { cand_t_ms = t; cand_tpl = tpl; }
        }
        if (!rc && cand_tpl && cand_t_ms < best_ms * 0.97f) { best_ms = cand_t_ms; best_tpl = cand_tpl; }
    } while (0);
    ws->defer_joins = saved_defer;
    if (rc == H2V_OK) set2(best_pair, best_tpl); else set2(saved_pair, saved_tpl);
    (void)hipStreamSynchronize(st);
    tmp.release();
    if (rc == H2V_OK && rep) {
        memset(rep, 0, sizeof *rep);
        rep->n_measured = n_meas; rep->default_ms = def_ms; rep->best_ms = best_ms; rep->calls_in_flight = depth;
        rep->pairing_engine = best_pair; rep->msm_terms_per_lane = best_tpl;
    }
    return rc;
}

// The record of the call `calls_back` calls before the most recent one on w (H2V_E_ARG: 64 or more back, or an earlier call's
// slot; a coalesced call whose group has not run yet has nothing to report).
static int rec_lookup(h2v_workspace *w, uint32_t calls_back, const CallRec **out) {
    const CallRec *r = calls_back < w->calls ? rec_at(w, w->calls - 1 - calls_back) : nullptr;
    if (!r) return fail(H2V_E_ARG, "no such call in the event ring");
    if (r->co && !r->ran) return fail(H2V_E_ARG, "that call is in a group of coalesced calls that has not run yet: h2v_workspace_join first");
    *out = r;
    return H2V_OK;
}
// The chunk walker of a laned workspace's record r: f(lane record) for chunk c = 0, 1, ... in order - chunk c ran on lane
// (first + c) % mod as that lane's record start[lane] + c / mod.  H2V_E_ARG when a lane has since given that record's slot to a
// later call.
template <class F> static int each_chunk(h2v_workspace *w, const CallRec &r, F &&f) {
    for (uint32_t c = 0; c < r.chunks; c++) {
        const uint32_t l = (r.first + c) % r.mod;
        const CallRec *lr = w->lane[l] ? rec_at(w->lane[l], r.start[l] + c / r.mod) : nullptr;
        if (!lr) return fail(H2V_E_ARG, "the lanes' event rings have wrapped since that call");
        if (int rc = f(*lr)) return rc;
    }
    return H2V_OK;
}
static int rec_timings(const CallRec &r, h2v_timings *tm);
// Per-kernel device times of a PAST call on this workspace (0 = the most recent, up to 63 back).  The events were
// recorded on the streams the kernels ran on; the caller must have synchronised the launch stream first.
extern "C" int h2v_workspace_timings(h2v_workspace *w, uint32_t calls_back, h2v_timings *tm) {
    if (!w || !tm) return fail(H2V_E_ARG, "null argument");
    ALIVE(w);
    const CallRec *r;
    if (int rc = rec_lookup(w, calls_back, &r)) return rc;
    if (r->kind == h2v_workspace::RLC && !r->routed) return fail(H2V_E_ARG, "that call ran in RLC mode: h2v_workspace_rlc_result");
    HIPCHK(hipSetDevice(w->device));
    if (!w->n_lanes) return rec_timings(*r, tm);
    // sums over the call's chunks (h2v_timings: `launches` = chunks); total_ms = first chunk's start .. the last end
    memset(tm, 0, sizeof *tm);
    hipEvent_t first = nullptr;
    int rc = each_chunk(w, *r, [&](const CallRec &lr) -> int {
        h2v_timings t1;
        if (int rc1 = rec_timings(lr, &t1)) return rc1;
        tm->transcript_combiner_ms += t1.transcript_combiner_ms; tm->g1_decompress_ms += t1.g1_decompress_ms;
        tm->g1_msm_ms += t1.g1_msm_ms; tm->pairing_ms += t1.pairing_ms; tm->g1_msm_fixed_ms += t1.g1_msm_fixed_ms;
        tm->msm_var_lanes_per_term = t1.msm_var_lanes_per_term;
        tm->msm_lanes_per_term = t1.msm_lanes_per_term; tm->pairing_lanes_per_proof = t1.pairing_lanes_per_proof;
        if (!first) first = lr.ev[2];
        float span = 0;
        HIPCHK(hipEventElapsedTime(&span, first, lr.ev[6]));
        if (span > tm->total_ms) tm->total_ms = span;
        return H2V_OK;
    });
    if (rc) return rc;
    tm->launches = r->chunks;
    if (r->co) {     // a coalesced call: its share of the one launch that served its group
        const float f = r->share;
        tm->transcript_combiner_ms *= f; tm->g1_decompress_ms *= f; tm->g1_msm_ms *= f; tm->pairing_ms *= f; tm->g1_msm_fixed_ms *= f;
    }
    return H2V_OK;
}
// the times of one record of an ordinary workspace (or of a lane)
static int rec_timings(const CallRec &r, h2v_timings *tm) {
    memset(tm, 0, sizeof *tm);
    tm->launches = 1;
    tm->msm_lanes_per_term = r.lpt;
    tm->pairing_lanes_per_proof = r.pair;
    const hipEvent_t *ev = r.ev;
    HIPCHK(hipEventSynchronize(ev[6]));
    HIPCHK(hipEventElapsedTime(&tm->transcript_combiner_ms, ev[0], ev[1]));
    HIPCHK(hipEventElapsedTime(&tm->g1_decompress_ms, ev[2], ev[3]));
    if (getenv("H2V_TIMELINE")) {
        fprintf(stderr, "[h2v timeline]");
        for (int q = 0; q < 7; q++) { float t; HIPCHK(hipEventElapsedTime(&t, ev[0], ev[q])); fprintf(stderr, " e%d=%.3f", q, t); }
        fprintf(stderr, "\n");
    }
    if (r.lpt == 3) {
        // split MSM: the ladder launch over the per-proof terms ([4] .. [9]) and, beside it on another stream, the
        // fixed-base launch over the VK-base terms ([7] .. [8]) - two kernels, two durations
        HIPCHK(hipEventElapsedTime(&tm->g1_msm_ms, ev[4], ev[9]));
        HIPCHK(hipEventElapsedTime(&tm->g1_msm_fixed_ms, ev[7], ev[8]));
        tm->msm_var_lanes_per_term = r.var_lpt;
    } else {
        HIPCHK(hipEventElapsedTime(&tm->g1_msm_ms, ev[4], ev[5]));
    }
    if (r.pair) HIPCHK(hipEventElapsedTime(&tm->pairing_ms, ev[5], ev[6]));   // (0: a prepare call - no pairing ran)
    HIPCHK(hipEventElapsedTime(&tm->total_ms, ev[2], ev[6]));
    return H2V_OK;
}

// The stream of the host-buffer entry points.  Not laned: it runs the kernels too - a pool stream (a hardware queue of its
// own).  Laned: it carries the uploads and the fork event only (and hs_down the downloads), the kernels run on the lanes'
// pool streams: plain non-blocking streams of the workspace, so that the copies never queue behind a lane's kernels - with
// eight two-stream lanes the pool's sixteen streams are all taken, and a pool stream shared with a lane held every upload
// back behind that lane's pairing launch (host path, 8 lanes: 877 k proofs/s; with its own copy streams: see DESIGN.md 6.1).
static int host_stream(h2v_workspace *ws) {
    if (!ws->hs) {
        if (ws->n_lanes) {
            HIPCHK(hipStreamCreateWithFlags(&ws->hs, hipStreamNonBlocking));
            ws->copy_streams_owned = true;
            if (!ws->hs_down) HIPCHK(hipStreamCreateWithFlags(&ws->hs_down, hipStreamNonBlocking));
        } else {
            HIPCHK(make_stream(&ws->hs));
        }
    }
    return H2V_OK;
}
using HostSlot = h2v_workspace::HostSlot;
// What a host-buffer form waits for before one of its blocks is freed: everything on `hs` - an earlier upload may still read the
// block, an earlier call's kernels write it - and, a mixed form (m given), every earlier mixed call on the workspace before that.
struct MixedWs;
static int mixed_quiesce(MixedWs *m);
static int host_quiet(h2v_workspace *ws, MixedWs *m) {
    if (m)
        if (int rc = mixed_quiesce(m)) return rc;
    HIPCHK(hipStreamSynchronize(ws->hs));
    return H2V_OK;
}
// THE packer of the host-buffer forms.  Packs the caller's batch into the pinned block of staging slot `sl` (hostcall::input_block:
// offsets | instances | committed | proofs; inst_bytes / ci_bytes size the two middle sections), enqueues ONE upload of it on
// ws->hs and returns the batch's device view in `in`.  Before a block that is too small is freed: an ordinary workspace's one
// slot (hslot[0]) waits for `hs`, a laned workspace's slot is free by construction, the mixed forms' slot (m given) waits as
// host_quiet says.
static int stage_batch(const h2v_batch *b, size_t inst_bytes, size_t ci_bytes, h2v_workspace *ws, HostSlot &sl, h2v_batch *in, MixedWs *m = nullptr) {
    const uint64_t n = b->n;
    if (!hostcall::offsets_ascend(n, b->proof_off)) return fail(H2V_E_ARG, "proof offsets must be non-decreasing");
    if (int rc = host_stream(ws)) return rc;
    const hostcall::InputBlock L = hostcall::input_block(n, inst_bytes, ci_bytes, b->proof_off[n] - b->proof_off[0]);
    auto quiet = [&]() { return ws->n_lanes && !m ? (int)H2V_OK : host_quiet(ws, m); };
    if (int rc = sl.in_block.ensure(sl.mem, L.need, "the staging block", quiet)) return rc;
    if (int rc = sl.h_block.ensure(sl.mem, L.need, "the staging block", quiet)) return rc;
    hostcall::pack_input(sl.h_block.p, L, n, b->proof_off, b->proofs, b->instances, b->committed);
    HIPCHK(hipMemcpyAsync(sl.in_block.p, sl.h_block.p, L.need, hipMemcpyHostToDevice, ws->hs));
    *in = {n, sl.in_block.p + L.proofs, (const uint64_t *)(sl.in_block.p + L.offsets), sl.in_block.p + L.inst, sl.in_block.p + L.ci};
    return H2V_OK;
}
// the slot a blocking form stages in (no batch is in flight: pairs_common): the ring's next slot, or the ordinary workspace's one
static HostSlot &own_slot(h2v_workspace *ws) { return ws->hslot[ws->n_lanes ? ws->h_head % h2v_workspace::MAXH : 0]; }
// (one key: the section sizes follow from the plan)
static int stage_batch(const h2v_plan *p, const h2v_batch *b, h2v_workspace *ws, HostSlot &sl, h2v_batch *in) {
    return stage_batch(b, (size_t)b->n * p->d.n_pi * 32, (size_t)b->n * p->d.n_ci * 48, ws, sl, in);
}
// A submitted batch: its slot's pinned download block (hostcall::accept_extent) and, laned, the device buffer its chunks write
// accept[] to (an ordinary workspace's is ws->accept) - the slot has no batch in flight, so nothing is waited for -, then the
// batch staged and u pointed at the device copy.
static int stage_unit(Unit &u, const h2v_batch *b, h2v_workspace *ws, HostSlot &sl) {
    const size_t need = hostcall::accept_extent(b->n);
    if (int rc = sl.h_accept.ensure(sl.mem, need, "the download block", no_wait)) return rc;
    if (ws->n_lanes)
        if (int rc = sl.d_accept.ensure(sl.mem, need, "the download block", no_wait)) return rc;
    h2v_batch in;
    if (int rc = stage_batch(u.p, b, ws, sl, &in)) return rc;
    u.proofs = in.proofs; u.off = in.proof_off; u.inst = in.instances; u.ci = in.committed;
    return H2V_OK;
}
// How many batch checks of the call just enqueued on ws failed - its record's word - comes down on `st`.  (Asynchronous: a
// synchronous copy would go through the legacy NULL stream, which every pool stream is ordered with, and drain all batches in flight.)
static int verdict_down(h2v_workspace *ws, void *dst, hipStream_t st) {
    if (hipMemcpyAsync(dst, rec_word(ws, rec_last(ws)), 4, hipMemcpyDeviceToHost, st) != hipSuccess) return fail(H2V_E_DEVICE, "download of the batch verdict failed");
    return H2V_OK;
}
// the results of the batch just enqueued into its slot's download block, on `st`: accept[n] and - a batch-check call - the verdict word
static int slot_download(h2v_workspace *ws, HostSlot &sl, const uint8_t *d_accept, hipStream_t st) {
    if (hipMemcpyAsync(sl.h_accept.p, d_accept, sl.n, hipMemcpyDeviceToHost, st) != hipSuccess) return fail(H2V_E_DEVICE, "download of accept[] failed");
    return sl.rlc ? verdict_down(ws, sl.h_accept.p + hostcall::accept_word(sl.n), st) : (int)H2V_OK;
}
// THE tail of the blocking host-buffer forms (prepare, pair check, aggregate, mixed), after the call was enqueued on ws->hs with
// its lanes joined and returned rc: every region of the result block with a destination comes down straight into the caller's
// memory (NULL - an optional output - is skipped), `verdict`: the record's word too, then ONE synchronise.  Any failure, the
// call's own included, returns through drain_after_error; otherwise fell_back (optional) = the batch check failed here or
// (also_failed) in a pass the call has already read the verdict of.
struct Down { void *dst; hostcall::Region from; const char *what; };
static int host_call_tail(h2v_workspace *ws, int rc, std::initializer_list<Down> downs, bool verdict, int *fell_back, const char *call, bool also_failed = false) {
    uint32_t failed = 0;
    for (const Down &d : downs)
        if (rc == H2V_OK && d.dst && hipMemcpyAsync(d.dst, ws->res.p + d.from.off, d.from.bytes, hipMemcpyDeviceToHost, ws->hs) != hipSuccess)
            rc = fail(H2V_E_DEVICE, std::string("download of ") + d.what + " failed");
    if (rc == H2V_OK && verdict) rc = verdict_down(ws, &failed, ws->hs);
    if (rc == H2V_OK && hipStreamSynchronize(ws->hs) != hipSuccess) rc = fail(H2V_E_DEVICE, std::string(call) + " kernels failed");
    if (rc) return drain_after_error(ws, rc);
    if (fell_back) *fell_back = (failed || also_failed) ? 1 : 0;
    return H2V_OK;
}
// The workspace's stream and its result block (ws->res) for one call of `kind` over n proofs; the block grows behind host_quiet.
static int result_ensure(h2v_workspace *ws, hostcall::Call kind, uint64_t n, hostcall::ResultBlock *R, MixedWs *m = nullptr) {
    if (int rc = host_stream(ws)) return rc;
    *R = hostcall::result_block(kind, n);
    return ws->res.ensure(ws->mem, R->extent, "the result block", [&]() { return host_quiet(ws, m); });
}
static bool rlc_supported(const h2v_plan *p);
static bool fold_pairs_wanted(const h2v_plan *p, const h2v_rlc_opts *o);
static int rlc_seed(const h2v_rlc_opts *o, uint32_t seed[8]);
static int seed_flags(const h2v_rlc_opts *o, bool *derive);
static int seed_flags_mixed(const h2v_rlc_opts *o, bool rlc, bool *keyed);

// Host-buffer batches on a LANED workspace: as many in flight as the mode has lanes, on ONE workspace.  Every batch gets a
// staging slot of its own (pinned block + device block + accept buffers); uploads run in order on `hs`, the chunks on
// the lanes, and the downloads on `hs_down`, each behind the lanes its batch ran on.  h2v_verify_batch_wait collects the
// OLDEST batch.  u: the call's kind and seed; its buffers are filled in here.
static int submit_laned(Unit u, const h2v_batch *b, h2v_workspace *ws) {
    const uint32_t depth = laned_depth(ws, b->n, u.kind == UnitKind::RLC, nullptr);
    if (ws->h_head - ws->h_tail >= depth || ws->h_head - ws->h_tail >= (uint64_t)h2v_workspace::MAXH)
        return fail(H2V_E_ARG, "as many batches in flight as this workspace has lanes: call h2v_verify_batch_wait first");
    if (!ws->hs_down) HIPCHK(make_stream(&ws->hs_down));
    h2v_workspace::HostSlot &sl = ws->hslot[ws->h_head % h2v_workspace::MAXH];
    if (int rce = lazy_event(sl.mem, sl.ev, hipEventDisableTiming)) return rce;
    const uint64_t n = b->n;
    sl.n = n; sl.rlc = u.batch_check();
    if (n) {
        if (int rcs = stage_unit(u, b, ws, sl)) return rcs;
        u.accept = sl.d_accept.p;
        int rc = run_call(u, ws, ws->hs, Join::NEVER);
        if (rc == H2V_OK) {
            // the download waits for the lanes this call's chunks ran on (their events as recorded just now)
            const CallRec &r = rec_last(ws);
            for (uint32_t c = 0; c < r.chunks && c < r.mod; c++)
                if (hipStreamWaitEvent(ws->hs_down, ws->lane_ev[(r.first + c) % r.mod], 0) != hipSuccess) rc = fail(H2V_E_DEVICE, "stream wait failed");
            if (rc == H2V_OK) rc = slot_download(ws, sl, sl.d_accept.p, ws->hs_down);
        }
        if (rc) return drain_after_error(ws, rc);
    }
    HIPCHK(hipEventRecord(sl.ev, ws->hs_down));
    ws->h_head++;
    ws->pending = true;
    return H2V_OK;
}
// A downloaded batch: accept bytes to the caller; fell_back (optional) = an RLC call whose record counted a failed batch check -
// the word that came back behind accept[] - so that the per-proof kernels produced accept[] (either kind of workspace)
static void host_results(const h2v_workspace::HostSlot &sl, uint8_t *accept, int *fell_back) {
    if (sl.n) memcpy(accept, sl.h_accept.p, sl.n);
    uint32_t failed = 0;
    if (sl.rlc && sl.n) memcpy(&failed, sl.h_accept.p + hostcall::accept_word(sl.n), 4);
    if (fell_back) *fell_back = failed ? 1 : 0;
}
static int wait_laned(h2v_workspace *ws, uint8_t *accept, int *fell_back) {
    if (ws->h_head == ws->h_tail) return fail(H2V_E_ARG, "no batch in flight on this workspace");
    h2v_workspace::HostSlot &sl = ws->hslot[ws->h_tail % h2v_workspace::MAXH];
    HIPCHK(hipEventSynchronize(sl.ev));
    host_results(sl, accept, fell_back);
    ws->h_tail++;
    ws->pending = ws->h_head != ws->h_tail;
    return H2V_OK;
}

// Asynchronous host-buffer form: packs + uploads the batch, enqueues the verification (per-proof, or the RLC batch mode
// with H2V_SUBMIT_RLC) and the download of accept[] on the workspace's stream, and returns.  The caller's buffers may be
// reused as soon as this returns (they were copied into pinned memory).  One batch at a time per workspace: alternate two
// workspaces to overlap the upload of batch k+1 with the kernels of batch k.
extern "C" int h2v_verify_batch_submit(const h2v_plan *p, const h2v_batch *b, h2v_workspace *ws, uint32_t flags, const h2v_rlc_opts *opts) {
    if (!p || !b || !ws) return fail(H2V_E_ARG, "null argument");
    ALIVE(p); ALIVE(ws);
    if (ws->pending && !ws->n_lanes) return fail(H2V_E_ARG, "the workspace already has a batch in flight: call h2v_verify_batch_wait first");
    if (b->n)
        if (int rca = batch_args(p, b)) return rca;
    HIPCHK(hipSetDevice(p->device));
    int rc = host_stream(ws);
    if (rc) return rc;
    if (b->n && (rc = ws_fits(ws, p, b->n, false))) return rc;
    const bool rlc = (flags & H2V_SUBMIT_RLC) && rlc_supported(p);
    const bool fold = (flags & H2V_SUBMIT_RLC) && !rlc && fold_pairs_wanted(p, opts);   // recursive plans: the batch check after the fold
    Unit u{fold ? UnitKind::FOLD_RLC : rlc ? UnitKind::RLC : UnitKind::VERIFY, p, (uint32_t)b->n};
    u.one_stream_opt = opts && (opts->flags & H2V_RLC_ONE_STREAM);
    bool derive = false;
    if ((flags & H2V_SUBMIT_RLC) && (rc = seed_flags(opts, &derive))) return rc;
    u.derive = derive && u.batch_check();
    if (ws->n_lanes) {
        if (u.batch_check() && !u.derive && (rc = rlc_seed(opts, u.seed))) return rc;
        return submit_laned(u, b, ws);
    }
    h2v_workspace::HostSlot &sl = ws->hslot[0];
    if (int rce = lazy_event(sl.mem, sl.ev, hipEventDisableTiming)) return rce;
    sl.n = b->n;
    sl.rlc = false;
    if (b->n) {
        if (u.batch_check() && !u.derive && (rc = rlc_seed(opts, u.seed))) return rc;
        if ((rc = stage_unit(u, b, ws, sl))) return rc;
        u.accept = ws->accept;
        rc = run_call(u, ws, ws->hs);
        sl.rlc = u.batch_check();
        if (rc == H2V_OK) rc = slot_download(ws, sl, ws->accept, ws->hs);
        if (rc) return drain_after_error(ws, rc);   // (the upload from the pinned block and some kernels may already be enqueued)
    }
    HIPCHK(hipEventRecord(sl.ev, ws->hs));
    ws->pending = true;
    return H2V_OK;
}
// Waits for the batch submitted on `ws`, copies its accept bytes out.  fell_back (optional): 1 when the batch was submitted
// in RLC mode and the batch check failed, so that the per-proof kernels produced accept[].
extern "C" int h2v_verify_batch_wait(h2v_workspace *ws, uint8_t *accept, int *fell_back) {
    if (!ws || !accept) return fail(H2V_E_ARG, "null argument");
    ALIVE(ws);
    if (ws->n_lanes) { HIPCHK(hipSetDevice(ws->device)); return wait_laned(ws, accept, fell_back); }
    if (!ws->pending) return fail(H2V_E_ARG, "no batch in flight on this workspace");
    HIPCHK(hipSetDevice(ws->device));
    ws->pending = false;
    const h2v_workspace::HostSlot &sl = ws->hslot[0];
    HIPCHK(hipEventSynchronize(sl.ev));
    host_results(sl, accept, fell_back);
    return H2V_OK;
}
static int verify_host(const h2v_plan *p, const h2v_batch *b, uint8_t *accept, h2v_workspace *ws, uint32_t flags, const h2v_rlc_opts *opts, int *fell_back) {
    if (!p || !b || !accept) return fail(H2V_E_ARG, "null argument");
    if (fell_back) *fell_back = 0;
    if (b->n == 0) return H2V_OK;
    ALIVE(p); ALIVE(ws);
    HIPCHK(hipSetDevice(p->device));
    TmpWs tmp;
    int rc = tmp.make(p, b->n, ws);
    if (rc == H2V_OK) rc = h2v_verify_batch_submit(p, b, ws, flags, opts);
    if (rc == H2V_OK) rc = h2v_verify_batch_wait(ws, accept, fell_back);
    return rc;
}
extern "C" int h2v_verify_batch(const h2v_plan *p, const h2v_batch *b, uint8_t *accept, h2v_workspace *ws) {
    return verify_host(p, b, accept, ws, 0, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------- prepare / pair check
// h2v_prepare_batch(_device): the verify pipeline up to the pairing, which k_prepare_export replaces (a PREPARE unit);
// h2v_check_pairs(_device): the pairing alone on pairs from anywhere (run_check).  Same argument rules as the verify calls;
// never gathered into coalesced groups (run_laned flushes the open groups first).
static int pairs_common(const h2v_plan *p, uint64_t n, h2v_workspace *&ws, const void *stream, bool device_form, TmpWs &tmp) {
    ALIVE(p); ALIVE(ws);
    HIPCHK(hipSetDevice(p->device));
    if (H2V_SLOTS(p->d) < 2) return fail(H2V_E_ARG, "internal: a plan with fewer than two point slots");
    if (int rc = tmp.make(p, n, ws)) return rc;
    int rc = ws_fits(ws, p, n, false);
    if (rc == H2V_OK && ws->pending) rc = fail(H2V_E_ARG, "the workspace has a host batch in flight: call h2v_verify_batch_wait first");
    if (rc == H2V_OK && device_form) rc = null_stream_check(ws, stream);
    return rc;
}
static int prepare_args(const h2v_plan *p, const h2v_batch *b, const uint8_t *pairs) {
    if (!p) return fail(H2V_E_ARG, "null argument: plan");
    if (!b) return fail(H2V_E_ARG, "null argument: batch");
    if (!pairs) return fail(H2V_E_ARG, "null argument: pairs");
    return H2V_OK;
}
static int pairs_args(const h2v_plan *p, const uint8_t *pairs, const uint8_t *accept) {
    if (!p) return fail(H2V_E_ARG, "null argument: plan");
    if (!pairs) return fail(H2V_E_ARG, "null argument: pairs");
    if (!accept) return fail(H2V_E_ARG, "null argument: accept");
    return H2V_OK;
}
extern "C" int h2v_prepare_batch_device(const h2v_plan *p, const h2v_batch *b, uint8_t *pairs, uint32_t *status, h2v_workspace *ws, void *stream) {
    if (int rc = prepare_args(p, b, pairs)) return rc;
    if (b->n == 0) return H2V_OK;
    if ((uintptr_t)pairs & 3) return fail(H2V_E_ARG, "pairs must be 4-byte aligned");
    if (int rc = batch_args(p, b)) return rc;
    TmpWs tmp;
    if (int rc = pairs_common(p, b->n, ws, stream, true, tmp)) return rc;
    Unit u = unit_of_batch(UnitKind::PREPARE, p, b, nullptr, status);
    u.pairs_out = pairs;
    return tmp.finish(run_call(u, ws, (hipStream_t)stream), (hipStream_t)stream);
}
extern "C" int h2v_check_pairs_device(const h2v_plan *p, uint64_t n, const uint8_t *pairs, uint8_t *accept, uint32_t *status, h2v_workspace *ws, void *stream) {
    if (int rc = pairs_args(p, pairs, accept)) return rc;
    if (n == 0) return H2V_OK;
    TmpWs tmp;
    if (int rc = pairs_common(p, n, ws, stream, true, tmp)) return rc;
    return tmp.finish(run_call(unit_of_pairs(UnitKind::CHECK, p, n, pairs, accept, status), ws, (hipStream_t)stream), (hipStream_t)stream);
}
// Host-buffer forms: the batch is staged as for h2v_verify_batch (pinned block, one upload on the workspace's stream), the
// call runs there with its lanes joined, and the outputs come back before the function returns.
extern "C" int h2v_prepare_batch(const h2v_plan *p, const h2v_batch *b, uint8_t *pairs, uint32_t *status, h2v_workspace *ws) {
    if (int rc = prepare_args(p, b, pairs)) return rc;
    if (b->n == 0) return H2V_OK;
    if (int rc = batch_args(p, b)) return rc;
    TmpWs tmp;
    if (int rc = pairs_common(p, b->n, ws, nullptr, false, tmp)) return rc;
    const uint64_t n = b->n;
    h2v_batch in{};
    hostcall::ResultBlock R;
    int rc = result_ensure(ws, hostcall::Call::PREPARE, n, &R);
    if (rc == H2V_OK) rc = stage_batch(p, b, ws, own_slot(ws), &in);
    if (rc) return rc;
    uint8_t *const d = ws->res.p;
    Unit u = unit_of_batch(UnitKind::PREPARE, p, &in, nullptr, (uint32_t *)(d + R.status.off));
    u.pairs_out = d + R.pairs.off;
    rc = run_call(u, ws, ws->hs, Join::NOW);
    return host_call_tail(ws, rc, {{pairs, R.pairs, "the pairs"}, {status, R.status, "the status words"}}, false, nullptr, "prepare");
}
// The host-buffer pair checks, u.kind CHECK (h2v_check_pairs) or PAIR_RLC (h2v_check_pairs_rlc: a seed, and the batch verdict
// comes back as fell_back): pairs up, the call with its lanes joined, accept[] / status[] down, all on the workspace's stream.
static int check_pairs_host(Unit u, const uint8_t *pairs, uint8_t *accept, uint32_t *status, h2v_workspace *ws, const h2v_rlc_opts *opts, int *fell_back) {
    const uint64_t n = u.n;
    const bool rlc = u.kind == UnitKind::PAIR_RLC;
    TmpWs tmp;
    if (int rc = pairs_common(u.p, n, ws, nullptr, false, tmp)) return rc;
    bool derive = false;
    int rc = rlc ? seed_flags(opts, &derive) : H2V_OK;
    u.derive = derive;
    if (rc == H2V_OK && rlc && !derive) rc = rlc_seed(opts, u.seed);
    hostcall::ResultBlock R;
    if (rc == H2V_OK) rc = result_ensure(ws, hostcall::Call::CHECK, n, &R);
    if (rc) return rc;
    uint8_t *const d = ws->res.p;
    u.pairs = d + R.pairs.off; u.accept = d + R.accept.off; u.status = (uint32_t *)(d + R.status.off);
    if (hipMemcpyAsync(d + R.pairs.off, pairs, R.pairs.bytes, hipMemcpyHostToDevice, ws->hs) != hipSuccess) rc = fail(H2V_E_DEVICE, "upload of the pairs failed");
    if (rc == H2V_OK) rc = run_call(u, ws, ws->hs, Join::NOW);
    return host_call_tail(ws, rc, {{accept, R.accept, "accept[]"}, {status, R.status, "the status words"}}, rlc, fell_back, "pair check");
}
extern "C" int h2v_check_pairs(const h2v_plan *p, uint64_t n, const uint8_t *pairs, uint8_t *accept, uint32_t *status, h2v_workspace *ws) {
    if (int rc = pairs_args(p, pairs, accept)) return rc;
    if (n == 0) return H2V_OK;
    return check_pairs_host(Unit{UnitKind::CHECK, p, (uint32_t)n}, pairs, accept, status, ws, nullptr, nullptr);
}


// ---------------------------------------------------------------------------------------------- bucket MSM (Pippenger)
// Device buffers of one bucket MSM over at most cap_n terms (h2v_pippenger.hpp).
struct PipWs {
    Owner mem;
    uint32_t cap_n = 0, cap_halves = 0;
    uint32_t *pts28 = nullptr, *cnt = nullptr, *off = nullptr, *order = nullptr, *cls = nullptr, *list = nullptr, *partial = nullptr, *wsum = nullptr;
    int16_t *dig = nullptr;
};
static void pip_free(PipWs &w) {
    w.mem.release();
    w = PipWs();
}
static int pip_alloc(PipWs &w, uint32_t cap_n, uint32_t halves) {
    const auto T = wslayout::bucket_msm(cap_n, halves);
    w.cap_n = cap_n; w.cap_halves = halves;
    const bool ok = w.mem.alloc(w.pts28, T.row[wslayout::B_PTS28]) && w.mem.alloc(w.dig, T.row[wslayout::B_DIG]) && w.mem.alloc(w.list, T.row[wslayout::B_LIST]) &&
                    w.mem.alloc(w.cnt, T.row[wslayout::B_CNT]) && w.mem.alloc(w.off, T.row[wslayout::B_OFF]) && w.mem.alloc(w.order, T.row[wslayout::B_ORDER]) &&
                    w.mem.alloc(w.cls, T.row[wslayout::B_CLS]) && w.mem.alloc(w.partial, T.row[wslayout::B_PARTIAL]) && w.mem.alloc(w.wsum, T.row[wslayout::B_WSUM]);
    if (!ok) { pip_free(w); return fail(H2V_E_DEVICE, "hipMalloc(bucket MSM workspace) failed"); }
    return H2V_OK;
}
// Window width for n terms.  Larger windows mean fewer windows (W = floor(128 / c) + 1 per GLV half) but 2^(c-1) buckets
// per window, capped at 512 so that one block's LDS holds a window in k_pip_reduce; at least ~24 entries per bucket on
// average.  chain = the most entries one lane of k_pip_accumulate sums (a bucket of more gets 2, 4, ... 256 lanes): short
// chains mean more lanes and deeper trees of complete additions.  H2V_OPT_RLC_WINDOW_BITS / _CHAIN force a shape (tests, tuning).
static void pip_shape(PipArgs &a) {
    const int env_c = g_opts.v[H2V_OPT_RLC_WINDOW_BITS], env_chain = g_opts.v[H2V_OPT_RLC_CHAIN];
    const double entries_per_window = (double)a.n * a.halves;
    uint32_t c = PIP_MAX_C;
    while (c > 4 && entries_per_window / (double)(1u << (c - 1)) < 24.0) c--;
    if (env_c >= 3 && env_c <= PIP_MAX_C) c = (uint32_t)env_c;
    a.c = c; a.NB = 1u << (c - 1); a.W = 128 / c + 1;
    while (a.W > PIP_MAX_W) { a.c++; a.NB <<= 1; a.W = 128 / a.c + 1; }
    a.chain = env_chain >= 2 && env_chain <= 1024 ? (uint32_t)env_chain : 20u;
}
static void pip_bind(const PipWs &w, PipArgs &a) {
    pip_shape(a);
    a.pts28 = w.pts28; a.dig = w.dig; a.cnt = w.cnt; a.off = w.off; a.order = w.order; a.cls = w.cls; a.list = w.list; a.partial = w.partial; a.wsum = w.wsum;
}
// Enqueues the six kernels of one or two bucket MSMs (np problems side by side in every launch) on `st`.
// a[]: n, halves, scal, pidx, pool0 / n_pool0 / pool1, out filled in; the shape (c, W, NB, chain) is filled in here.  ev (optional):
// 4 events recorded at the start, before and after k_pip_accumulate, and at the end.  acc_grid_cap (test-only, 0 = none: what every
// production call passes) caps the grid of k_pip_accumulate below the host's estimate, so that its blocks walk several logical
// blocks each; acc_blocks_out (optional) receives the number of blocks that launch had.
static int pip_launch(const PipWs *const *ws, PipArgs *a, uint32_t np, hipStream_t st, hipEvent_t *ev, uint32_t acc_grid_cap = 0,
                      uint32_t *acc_blocks_out = nullptr) {
    PipArgs2 a2 = {};
    uint32_t max_n = 0, max_W = 0, max_NB = 0, max_acc_blocks = 0;
    for (uint32_t q = 0; q < np; q++) {
        if (a[q].n > ws[q]->cap_n || a[q].halves > ws[q]->cap_halves) return fail(H2V_E_ARG, "bucket MSM workspace too small");
        pip_bind(*ws[q], a[q]);
        a2.p[q] = a[q];
        const uint32_t nb = a[q].W * a[q].NB;
        // lanes of k_pip_accumulate: a bucket of count cnt > T gets fewer than 2 cnt / T lanes, any other non-empty one 1; each
        // class is padded to whole blocks
        const uint64_t lanes = 2ull * a[q].n * a[q].halves * a[q].W / a[q].chain + nb + 256ull * PIP_N_CLASSES;
        max_n = a[q].n > max_n ? a[q].n : max_n; max_W = a[q].W > max_W ? a[q].W : max_W; max_NB = a[q].NB > max_NB ? a[q].NB : max_NB;
        const uint32_t blocks = (uint32_t)((lanes + 255) / 256);
        max_acc_blocks = blocks > max_acc_blocks ? blocks : max_acc_blocks;
    }
    if (acc_grid_cap && acc_grid_cap < max_acc_blocks) max_acc_blocks = acc_grid_cap;
    if (acc_blocks_out) *acc_blocks_out = max_acc_blocks;
    if (ev) HIPCHK(hipEventRecord(ev[0], st));
    for (uint32_t q = 0; q < np; q++) HIPCHK(hipMemsetAsync(a[q].cnt, 0, (size_t)a[q].W * a[q].NB * 4, st));
    if (max_n) hipLaunchKernelGGL(k_pip_digits, dim3((max_n + 255) / 256, np), dim3(256), 0, st, a2);
    hipLaunchKernelGGL(k_pip_scan, dim3(1, np), dim3(1024), 0, st, a2);
    if (max_n) hipLaunchKernelGGL(k_pip_scatter, dim3((max_n + 255) / 256, np), dim3(256), 0, st, a2);
    if (ev) HIPCHK(hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(k_pip_accumulate, dim3(max_acc_blocks, np), dim3(256), 0, st, a2);
    if (ev) HIPCHK(hipEventRecord(ev[2], st));
    const size_t lds = (size_t)43 * max_NB * 4;
    HIPCHK(hipFuncSetAttribute((const void *)k_pip_reduce, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_pip_reduce, dim3(max_W, np), dim3(max_NB), lds, st, a2);
    hipLaunchKernelGGL(k_pip_combine, dim3(1, np), dim3(64), 0, st, a2);
    if (ev) HIPCHK(hipEventRecord(ev[3], st));
    HIPCHK(hipGetLastError());
    return H2V_OK;
}

// ---------------------------------------------------------------------------------------------- RLC batch mode
struct RlcWs {
    Owner mem;                  // of the set's own blocks; the bucket-MSM sets R and L and the group stage own theirs
    uint64_t cap = 0;
    uint32_t n_var = 0, n_fix = 0;
    uint32_t *r_scal = nullptr, *r_idx = nullptr, *l_scal = nullptr, *l_idx = nullptr, *vk_part = nullptr;
    uint8_t *good = nullptr;
    uint32_t *pool = nullptr;   // the pair-RLC set, H2V_RLC_FOLD_PAIRS: cap two-slot records of folded pairs (k_fold_pairs_affine)
    PipWs R, L;
    uint32_t *sums = nullptr;   // er (36 dwords) then el (36): the two MSM results
    uint32_t *misc = nullptr;   // [0..23] a dummy affine point, [24] status of the batch check, [26] its valid byte, [27] its accept byte
    uint32_t *flags = nullptr;  // [0] the batch check passed, [1 + g] group g (proofs 64 g ..) is final: cap / 64 + 2 dwords
    uint32_t *fold_rpts = nullptr, *fold_lpts = nullptr;   // the fold form of a mixed call: the COPIED points of the terms (24 dwords each)
    // fall-back stage 1 (group checks, created by the first call with at least GRP_MIN_N proofs): term lists, sums and
    // verdict buffers of the groups, the argument array of their 2 G bucket MSMs and ONE pool for those MSMs' buffers
    struct Grp {
        Owner mem;
        uint32_t n = 0, G = 0, stride = 0, max_n = 0, acc_blocks = 0;
        uint64_t key_gen = 0;          // the plan (load counter) the cached arguments were built for
        const uint32_t *key_pts = nullptr;
        uint32_t cap_stride = 0;
        void *staged[8] = {};          // pinned host copies of argument arrays whose uploads may still be in flight
        uint32_t n_staged = 0;
        uint32_t *g_scal = nullptr, *g_idx = nullptr, *er_g = nullptr, *el_g = nullptr, *pts_g = nullptr, *status_g = nullptr;
        uint8_t *valid_g = nullptr, *accept_g = nullptr, *pool = nullptr;
        PipArgs *args_d = nullptr;
        size_t cnt_bytes = 0;
        uint32_t cap_G = 0;
    } grp;
};
static void rlc_release(RlcWs *r) {      // (the caller has drained the streams: ws_release, or waited for the set's users)
    r->mem.release(); r->grp.mem.release();
    pip_free(r->R); pip_free(r->L);
    delete r;
}
// THE allocator of an RlcWs, in the set's three shapes (h2v_ws_layout.hpp: rlc_plan, rlc_pairs, rlc_fold).  Pairs have 128-bit
// scalars on both sides and no left-hand array of their own (l_scal = r_scal).
static RlcWs *rlc_new(uint64_t cap, uint32_t n_var, uint32_t n_fix, const wslayout::RlcSet &S) {
    RlcWs *r = new RlcWs();
    r->cap = cap; r->n_var = n_var; r->n_fix = n_fix;
    const auto &T = S.t;
    bool ok = r->mem.alloc(r->r_scal, T.row[wslayout::R_R_SCAL]) && r->mem.alloc(r->r_idx, T.row[wslayout::R_R_IDX]) && r->mem.alloc(r->l_scal, T.row[wslayout::R_L_SCAL]) &&
              r->mem.alloc(r->l_idx, T.row[wslayout::R_L_IDX]) && r->mem.alloc(r->vk_part, T.row[wslayout::R_VK_PART]) && r->mem.alloc(r->good, T.row[wslayout::R_GOOD]) &&
              r->mem.alloc(r->sums, T.row[wslayout::R_SUMS]) && r->mem.alloc(r->misc, T.row[wslayout::R_MISC]) && r->mem.alloc(r->flags, T.row[wslayout::R_FLAGS]) &&
              r->mem.alloc(r->fold_rpts, T.row[wslayout::R_FOLD_RPTS]) && r->mem.alloc(r->fold_lpts, T.row[wslayout::R_FOLD_LPTS]);
    if (ok && !r->l_scal) r->l_scal = r->r_scal;
    if (ok) ok = pip_alloc(r->R, S.r_cap_n, S.r_halves) == H2V_OK && pip_alloc(r->L, S.l_cap_n, 1) == H2V_OK;
    if (!ok) { rlc_release(r); return nullptr; }
    return r;
}
// One set of buffers per plan SHAPE (n_var, n_fix) the workspace has served: a workspace that alternates between plans (ws_fits
// allows any plan that fits; h2v_workspace_create_multi is made for it) swaps between parked sets instead of freeing and
// re-allocating at every switch - hipFree waits for the whole device.  At most eight shapes are kept.
static int rlc_ensure(h2v_workspace *w, const h2v_plan *p) {
    if (w->rlc && w->rlc->n_var == p->n_var && w->rlc->n_fix == p->n_fix) return H2V_OK;
    for (size_t k = 0; k < w->rlc_parked.size(); k++) {
        RlcWs *q = w->rlc_parked[k];
        if (q->n_var == p->n_var && q->n_fix == p->n_fix) {
            w->rlc_parked[k] = w->rlc;
            if (!w->rlc_parked[k]) w->rlc_parked.erase(w->rlc_parked.begin() + (long)k);
            w->rlc = q;
            return H2V_OK;
        }
    }
    if (w->rlc) {
        if (w->rlc_parked.size() >= 8) { rlc_release(w->rlc_parked.front()); w->rlc_parked.erase(w->rlc_parked.begin()); }
        w->rlc_parked.push_back(w->rlc);
        w->rlc = nullptr;
    }
    RlcWs *r = rlc_new(w->cap, p->n_var, p->n_fix, wslayout::rlc_plan(w->cap, p->n_var, p->n_fix));
    if (!r) return fail(H2V_E_DEVICE, "RLC workspace allocation failed");
    w->rlc = r;
    return H2V_OK;
}
// The pair-RLC set of a workspace or lane (h2v_check_pairs_rlc, H2V_RLC_FOLD_PAIRS), sized by its capacity and allocated at
// the first such call: the shape "one variable term per pair, no VK base" of the same buffers - one scalar array for both sums,
// the index arrays 2 i / 2 i + 1, good, sums, flags, two bucket-MSM workspaces of 128-bit scalars.  with_pool: the folded pairs' own pool.
static int pair_rlc_ensure(h2v_workspace *w, bool with_pool) {
    if (!w->prlc && !(w->prlc = rlc_new(w->cap, 1, 0, wslayout::rlc_pairs(w->cap)))) return fail(H2V_E_DEVICE, "pair-RLC workspace allocation failed");
    if (with_pool && !w->prlc->pool && !w->prlc->mem.alloc(w->prlc->pool, wslayout::rlc_pair_pool(w->cap)))
        return fail(H2V_E_DEVICE, "pair-RLC workspace allocation failed");
    return H2V_OK;
}
static bool rlc_supported(const h2v_plan *p) { return !p->d.ivc && p->n_var > 0 && p->n_fix > 0 && p->n_var + p->n_fix == p->d.n_terms; }

// Fall-back stage 1: group checks (h2v_rlc.hpp: k_rlc_group_terms, k_pairing_rlc_groups).  Groups of 64 proofs; every group
// is two small bucket MSMs (right: 64 n_var + n_fix terms, 255-bit scalars; left: 64 terms, 128-bit) with 7-bit windows
// (64 buckets x 19 windows: ~20 entries per bucket on the right).  Batches below GRP_MIN_N proofs or above GRP_MAX_G groups
// go straight to the per-proof kernels.  Everything here is enqueued behind the batch check and returns at once when it
// passed.  H2V_OPT_RLC_GROUP_STAGE = -1 switches the stage off (measurements).  (Window width 5 / 6 / 7 / 8 bits, one rejecting proof per
// 4096-proof batch, sixteen batches in flight: 2.90 / 2.72 / 2.86 / 2.80 ms per batch - the three pairing stages in a row are
// what the fall-back waits for, not these sums.)
#define GRP_MIN_N 256u
#define GRP_MAX_G 512u
using wslayout::GRP_C;      // (window bits of the group stage: its pool is laid out in h2v_ws_layout.hpp)
static bool rlc_groups_on(uint32_t n) {
    return g_opts.v[H2V_OPT_RLC_GROUP_STAGE] >= 0 && n >= GRP_MIN_N && (n + 63) / 64 <= GRP_MAX_G;
}
// The argument array of the group stage is cached per (batch size, plan, point buffer).  When it has to change, the new one
// is uploaded ON THE CALL'S STREAM from a pinned host copy: the kernels of an earlier call on that stream read args_d when
// they run, and a synchronous hipMemcpy (through the NULL stream, not ordered with a non-blocking caller stream) could
// hand them the new batch size's pointers.  The key is the plan's load counter, not its address.
// GrpShape: what the stage sums over - the proofs of a plan (grp_of_plan: its per-proof terms out of the workspace's point
// buffer, then its VK bases; 255-bit scalars on the right) or pairs (grp_of_pairs: one term per pair out of `pool`, no VK base,
// 128-bit scalars on both sides).
struct GrpShape { uint32_t n_var, n_fix, slots, halves; const uint32_t *pool, *vk_bases, *terms; uint64_t gen; };
static GrpShape grp_of_plan(const h2v_plan *p, const h2v_workspace *w) { return {p->n_var, p->n_fix, (uint32_t)H2V_SLOTS(p->d), 2, w->pts, p->d.vk_bases, p->d.terms, p->gen}; }
static GrpShape grp_of_pairs(const h2v_plan *p, const uint32_t *pool) { return {1, 0, 2, 1, pool, nullptr, nullptr, p->gen}; }
static int rlc_groups_ensure(RlcWs *r, const GrpShape &gs, uint32_t n, hipStream_t st) {
    RlcWs::Grp &g = r->grp;
    const uint32_t G = (n + 63) / 64, slots = gs.slots;
    const uint32_t W = 128 / GRP_C + 1, NB = 1u << (GRP_C - 1), nb = W * NB, stride = 64 * gs.n_var + gs.n_fix;
    if (g.n == n && g.key_gen == gs.gen && g.key_pts == gs.pool && g.stride == stride) return H2V_OK;
    if (G > g.cap_G || stride > g.cap_stride) {
        HIPCHK(hipStreamSynchronize(st));     // (the buffers about to be freed may be in use by the previous call)
        g.mem.release();
        g = RlcWs::Grp();
        const auto T = wslayout::group_stage(G, stride);
        const bool ok = g.mem.alloc(g.g_scal, T.row[wslayout::G_SCAL]) && g.mem.alloc(g.g_idx, T.row[wslayout::G_IDX]) && g.mem.alloc(g.er_g, T.row[wslayout::G_ER]) &&
                        g.mem.alloc(g.el_g, T.row[wslayout::G_EL]) && g.mem.alloc(g.pts_g, T.row[wslayout::G_PTS]) && g.mem.alloc(g.status_g, T.row[wslayout::G_STATUS]) &&
                        g.mem.alloc(g.valid_g, T.row[wslayout::G_VALID]) && g.mem.alloc(g.accept_g, T.row[wslayout::G_ACCEPT]) && g.mem.alloc(g.pool, T.row[wslayout::G_POOL]) &&
                        g.mem.alloc(g.args_d, T.row[wslayout::G_ARGS]);
        if (!ok) return fail(H2V_E_DEVICE, "hipMalloc(RLC group stage) failed");
        g.cap_G = G; g.cap_stride = stride;
    }
    // the argument array: problem 2 q = the right-hand sum of group q, 2 q + 1 its left-hand sum; their buffers lie in the pool
    // where wslayout::group_pool says.  The pool was sized by the same function for cap_G groups of cap_stride terms in two halves,
    // the counters of all cap_G groups come first, and a region only shrinks with the stride and the halves: groups q < G <= cap_G
    // of this call's stride end inside it (tests/cpp/h2v_ws_layout.cpp binds every region of a pool of exactly the total)
    const wslayout::GroupPool lay = wslayout::group_pool(g.cap_G, stride, gs.halves);
    g.cnt_bytes = lay.cnt_bytes;
    std::vector<PipArgs> args(2 * (size_t)G);
    uint32_t max_n = 0, acc_blocks = 1;
    for (uint32_t q = 0; q < G; q++) {
        const uint32_t ng = n - q * 64 < 64 ? n - q * 64 : 64;
        for (int side = 0; side < 2; side++) {
            PipArgs a = {};
            a.c = GRP_C; a.W = W; a.NB = NB; a.chain = 20;
            a.pool0 = gs.pool; a.n_pool0 = n * slots;
            if (side == 0) {
                a.n = ng * gs.n_var + gs.n_fix; a.halves = gs.halves;
                a.scal = g.g_scal + (size_t)q * stride * 8; a.pidx = g.g_idx + (size_t)q * stride; a.pool1 = gs.vk_bases; a.out = g.er_g + (size_t)q * 36;
            } else {
                a.n = ng; a.halves = 1;
                a.scal = r->l_scal + (size_t)q * 64 * 8; a.pidx = r->l_idx + (size_t)q * 64; a.pool1 = nullptr; a.out = g.el_g + (size_t)q * 36;
            }
            const wslayout::GroupPool::At at = lay.at(q, side);
            a.cnt = (uint32_t *)(g.pool + at.cnt); a.pts28 = (uint32_t *)(g.pool + at.pts28); a.dig = (int16_t *)(g.pool + at.dig);
            a.list = (uint32_t *)(g.pool + at.list); a.off = (uint32_t *)(g.pool + at.off); a.order = (uint32_t *)(g.pool + at.order);
            a.cls = (uint32_t *)(g.pool + at.cls); a.partial = (uint32_t *)(g.pool + at.partial); a.wsum = (uint32_t *)(g.pool + at.wsum);
            args[2 * q + side] = a;
            max_n = a.n > max_n ? a.n : max_n;
            const uint64_t lanes = 2ull * a.n * a.halves * W / a.chain + nb + 256ull * PIP_N_CLASSES;
            const uint32_t blocks = (uint32_t)((lanes + 255) / 256);
            acc_blocks = blocks > acc_blocks ? blocks : acc_blocks;
        }
    }
    if (g.n_staged >= 8) {                    // (a workspace whose batch size keeps alternating: drain, then reuse)
        HIPCHK(hipStreamSynchronize(st));
        for (void *&q : g.staged) g.mem.drop(q);
        g.n_staged = 0;
    }
    void *&pinned = g.staged[g.n_staged];
    if (!g.mem.alloc_pinned(pinned, wslayout::group_args_bytes(G))) return fail(H2V_E_DEVICE, "staging allocation failed");
    g.n_staged++;
    memcpy(pinned, args.data(), args.size() * sizeof(PipArgs));
    HIPCHK(hipMemcpyAsync(g.args_d, pinned, args.size() * sizeof(PipArgs), hipMemcpyHostToDevice, st));   // behind the earlier call's kernels
    g.n = n; g.G = G; g.stride = stride; g.max_n = max_n; g.acc_blocks = acc_blocks; g.key_gen = gs.gen; g.key_pts = gs.pool;
    return H2V_OK;
}
// stats: the workspace's failing-group counters, or NULL (pairs: that estimate describes proofs of a plan)
static int rlc_groups_launch(RlcWs *r, const GrpShape &gs, uint32_t n, uint8_t *accept, const H2vDevPlan &d1, hipStream_t st, uint32_t *stats) {
    int rc = rlc_groups_ensure(r, gs, n, st);
    if (rc) return rc;
    RlcWs::Grp &g = r->grp;
    const uint32_t G = g.G;
    RlcGroupArgs ga = {n, gs.n_var, gs.n_fix, gs.slots, g.stride, gs.terms, r->r_scal, r->r_idx, r->vk_part, g.g_scal, g.g_idx};
    hipLaunchKernelGGL(k_rlc_group_terms, dim3(G), dim3(64), 0, st, ga, r->flags);
    HIPCHK(hipMemsetAsync(g.pool, 0, g.cnt_bytes, st));
    HIPCHK(hipMemsetAsync(g.status_g, 0, (size_t)G * 4, st));
    hipLaunchKernelGGL(k_pip_digits_many, dim3((g.max_n + 255) / 256, 2 * G), dim3(256), 0, st, g.args_d, r->flags);
    hipLaunchKernelGGL(k_pip_scan_many, dim3(1, 2 * G), dim3(1024), 0, st, g.args_d, r->flags);
    hipLaunchKernelGGL(k_pip_scatter_many, dim3((g.max_n + 255) / 256, 2 * G), dim3(256), 0, st, g.args_d, r->flags);
    hipLaunchKernelGGL(k_pip_accumulate_many, dim3(g.acc_blocks, 2 * G), dim3(256), 0, st, g.args_d, r->flags);
    const uint32_t Wg = 128 / GRP_C + 1;
    hipLaunchKernelGGL(k_pip_wsum_many, dim3((2 * G * Wg * 4 + 63) / 64), dim3(64), 0, st, g.args_d, 2 * G, Wg, r->flags);
    hipLaunchKernelGGL(k_pip_horner_many, dim3(2 * G), dim3(64), 0, st, g.args_d, r->flags);
    hipLaunchKernelGGL(k_pairing_rlc_groups, dim3(G), dim3(64), COOP_LDS_BYTES(1), st, d1, g.pts_g, g.valid_g, g.er_g, g.el_g, g.status_g, g.accept_g, G, n,
                       r->good, accept, r->flags, stats);
    HIPCHK(hipGetLastError());
    return H2V_OK;
}

// ONE pairing check for the batch over a one-proof view of the plan: el = L = r->sums + 36, er = R = r->sums (both Jacobian), no
// per-proof points; ev9 marks its end.  Behind it - skipped on the device when the check passed - the group stage over gs.
// fail_ctr: the unit's, or NULL: the record's word, zeroed here.  stats: the failing-group counters, or NULL (pairs: that
// estimate describes proofs of a plan).  Everything behind it takes r->flags as skip flags.  group_stage = false: the check
// alone (the fold form of a mixed call: a group of 64 call positions spans plans, so no group term list applies).
static int launch_batch_pairing(const Unit &u, RlcWs *r, const GrpShape &gs, uint32_t *stats, h2v_workspace *w, CallRec &rec, hipStream_t st,
                                bool group_stage = true) {
    const uint32_t n = u.n;
    H2vDevPlan d1 = u.p->d;
    d1.n_points = 1; d1.n_ci = 0; d1.ivc = 0; d1.pi_point = 0;
    uint32_t *st1 = r->misc + 24, *fail_ctr = u.fail_ctr;
    uint8_t *valid1 = (uint8_t *)(r->misc + 26), *acc1 = (uint8_t *)(r->misc + 27);
    HIPCHK(hipMemsetAsync(st1, 0, 4, st));            // status of the batch check
    HIPCHK(hipMemsetAsync(valid1, 1, 1, st));
    if (!fail_ctr) {
        fail_ctr = rec_word(w, rec);
        HIPCHK(hipMemsetAsync(fail_ctr, 0, 4, st));
    }
    hipLaunchKernelGGL(k_pairing_rlc, dim3(1), dim3(64), COOP_LDS_BYTES(1), st, d1, r->misc, valid1, r->sums, r->sums + 36, st1, acc1, n, r->good, u.accept, r->flags,
                       (n + 63) / 64, fail_ctr, stats, group_stage && rlc_groups_on(n) ? 1u : 0u);
    HIPCHK(hipEventRecord(rec.ev[9], st));
    if (group_stage && rlc_groups_on(n))
        if (int rc = rlc_groups_launch(r, gs, n, u.accept, d1, st, stats)) return rc;
    return H2V_OK;
}
// The end of a unit of an AGGREGATE call, in place of launch_batch_pairing and everything its callers queue behind it: good_i to the
// caller's included[] (u.accept, the unit's range of it), the unit's two sums (r->sums: R, then L, Jacobian) to its part of the
// call's parts buffer - a lane's r->sums is overwritten by its next chunk -, ev[9] for the record's times.  The record's verdict
// word stays 0 and means nothing: h2v_workspace_rlc_result reports H2V_BATCH_NOT_CHECKED for a record with `agg` set.
static int agg_chunk(const Unit &u, RlcWs *r, h2v_workspace *w, CallRec &rec, hipStream_t st) {
    rec.agg = true;
    if (!u.fail_ctr) HIPCHK(hipMemsetAsync(rec_word(w, rec), 0, 4, st));
    HIPCHK(hipMemcpyAsync(u.accept, r->good, u.n, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(u.agg_parts + (size_t)u.part * AGG_PART_DW, r->sums, AGG_PART_DW * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipEventRecord(rec.ev[9], st));
    return H2V_OK;
}
// PHASE 1 of a batch-accept unit (run_rlc, run_mixed_terms, run_mixed_group): the decompression on the workspace's side stream,
// forked from `st` and joined back into it, the combiner beside it on `st`; one_stream (each caller's own rule): both on `st`,
// the decompression first.  dec_ev / comb_ev: the record's two events around each.  decompress(stream) / combine(stream) enqueue
// the launch(es) and return a code.
template <class Dec, class Comb>
static int phase1(h2v_workspace *w, hipStream_t st, bool one_stream, const hipEvent_t *dec_ev, const hipEvent_t *comb_ev, Dec &&decompress, Comb &&combine) {
    if (!one_stream)
        if (int rc = ws_streams(w, false, true)) return rc;
    hipStream_t ps = one_stream ? st : w->pside;
    if (!one_stream) {
        HIPCHK(hipEventRecord(w->ev_fork, st));
        HIPCHK(hipStreamWaitEvent(ps, w->ev_fork, 0));
    }
    HIPCHK(hipEventRecord(dec_ev[0], ps));
    if (int rc = decompress(ps)) return rc;
    HIPCHK(hipEventRecord(dec_ev[1], ps));
    HIPCHK(hipEventRecord(w->ev_join, ps));
    HIPCHK(hipEventRecord(comb_ev[0], st));
    if (int rc = combine(st)) return rc;
    HIPCHK(hipEventRecord(comb_ev[1], st));
    if (!one_stream) HIPCHK(hipStreamWaitEvent(st, w->ev_join, 0));
    return H2V_OK;
}
// THE SUMS of a batch check, R and L side by side in the same six bucket-MSM launches (pip_launch; the record's ev[5..8]), into
// r->sums (R, then L at + 36).  A sum: n terms of scalars scal (halves = 2: 255 bits, GLV; 1: below 2^128), term t the point
// pidx[t] (NULL: t) of pool0 (n_pool0 points) and, behind those, of pool1.  The record keeps R's shape for the timings.
struct SumTerms { uint32_t n, halves; const uint32_t *scal, *pidx, *pool0; uint32_t n_pool0; const uint32_t *pool1; };
static int launch_sums(RlcWs *r, const SumTerms &R, const SumTerms &L, CallRec &rec, hipStream_t st) {
    PipArgs pa[2] = {};
    const SumTerms *s[2] = {&R, &L};
    for (int q = 0; q < 2; q++) {
        pa[q].n = s[q]->n; pa[q].halves = s[q]->halves; pa[q].scal = s[q]->scal; pa[q].pidx = s[q]->pidx;
        pa[q].pool0 = s[q]->pool0; pa[q].n_pool0 = s[q]->n_pool0; pa[q].pool1 = s[q]->pool1; pa[q].out = r->sums + 36 * q;
    }
    const PipWs *pws[2] = {&r->R, &r->L};
    if (int rc = pip_launch(pws, pa, 2, st, rec.ev + 5)) return rc;   // ev[5..8]
    rec.rlc_c = pa[0].c; rec.rlc_W = pa[0].W; rec.rlc_chain = pa[0].chain; rec.rlc_terms = pa[0].n;
    return H2V_OK;
}
// One batch in RLC mode.  Phase 1 as in run_pipeline (the decompression launch builds no window tables), then the batch
// check; the per-proof MSM + pairing kernels are queued behind it and return at once unless the batch check failed.
// Events (the record's): [0]/[1] around the decompression, [2]/[3] around the
// combiner, [10]/[4] around the scalar preparation, [5] .. [8] the bucket MSMs (pip_launch), [8]/[9] around the pairing.
static int run_rlc(const Unit &u, h2v_workspace *w, hipStream_t st) {
    const h2v_plan *p = u.p;
    const H2vDevPlan &d = p->d;
    const uint32_t n = u.n;
    int rc = rlc_ensure(w, p);
    if (rc) return rc;
    LaunchOptsScope opts(w);
    RlcWs *r = w->rlc;
    const uint32_t slots = H2V_SLOTS(d);
    CallRec &rec = rec_new(w, h2v_workspace::RLC);
    hipEvent_t *ev = rec.ev;
    // two streams per batch: the caller's (transcript + combiner, then everything else) and one for the decompression
    // one_stream (h2v_rlc_opts.flags & H2V_RLC_ONE_STREAM, or H2V_OPT_STREAMS = 1): everything on
    // the caller's stream, decompression before the combiner - one stream per batch in flight instead of two
    const bool one_stream = w->one_stream_mode >= 0 ? w->one_stream_mode != 0 : (u.one_stream_opt || w->in_flight_hint >= 3);   // (H2V_OPT_STREAMS, the flag, or the caller's in-flight hint)
    hipStream_t pm = st;
    rc = phase1(w, st, one_stream, ev + 0, ev + 2,
                [&](hipStream_t ps) { return launch_decompress(d, n, u.proofs, u.off, u.ci, u.inst, w, nullptr, ps); },
                [&](hipStream_t s) { return launch_vm(d, n, w->stride, u.proofs, u.off, u.inst, u.ci, w->regs, w->scalars, w->status, nullptr, s); });
    if (rc) return rc;
    HIPCHK(hipEventRecord(ev[10], pm));
    // the batch check
    RlcArgs ra = {n, p->n_var, p->n_fix, slots, d.pi_point, d.n_terms, d.terms, w->scalars, w->status, w->valid, w->valid_sub, {},
                  r->r_scal, r->r_idx, r->l_scal, r->l_idx, r->vk_part, r->good, u.seed_dev, u.seed_xor7};
    copy_seed(ra.seed, u.seed);
    const uint32_t blocks = (n + 63) / 64;
    hipLaunchKernelGGL(k_rlc_prepare, dim3(blocks), dim3(64), 0, pm, ra);
    hipLaunchKernelGGL(k_rlc_vk_sum, dim3((p->n_fix + 63) / 64), dim3(64), 0, pm, ra, blocks);
    HIPCHK(hipEventRecord(ev[4], pm));
    // both sums in the same launches: R = sum r_i er_i (255-bit scalars, GLV) and L = sum r_i pi_i (128-bit scalars)
    if ((rc = launch_sums(r, {n * p->n_var + p->n_fix, 2, r->r_scal, r->r_idx, w->pts, n * slots, d.vk_bases}, {n, 1, r->l_scal, r->l_idx, w->pts, n * slots, nullptr}, rec, pm)))
        return rc;
    if (u.agg_parts) {      // an aggregate call stops here: no pairing, no group stage, no per-proof kernels
        if ((rc = agg_chunk(u, r, w, rec, pm))) return rc;
        if (u.status) HIPCHK(hipMemcpyAsync(u.status, w->status, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
        return H2V_OK;
    }
    // fall-back, skipped on the device when the batch check passed.  Stage 1 finds the groups of 64 proofs that hold a failing
    // proof (everything else is final); stage 2 - window tables, per-proof MSM, per-proof pairing - decides inside those
    // groups.  Walking grids of one wave per SIMD: finding out that a launch is not needed costs a few microseconds, and a
    // launch that IS needed has the whole chip.
    if ((rc = launch_batch_pairing(u, r, grp_of_plan(p, w), w->rlc_stats_ptr ? w->rlc_stats_ptr : w->rlc_stats, w, rec, pm))) return rc;
    uint32_t *skip = r->flags;
    const uint32_t cond_grid = (uint32_t)(msm_n_simd() / 4.0);
    {
        const uint32_t nb = (n * slots + 63) / 64;
        hipLaunchKernelGGL(k_build_tables, dim3(nb < 4 * cond_grid ? nb : 4 * cond_grid), dim3(64), 0, pm, n * slots, w->pts, w->valid, w->pt_tab, skip, slots);
    }
    {
        H2vMsmArgs ma = msm_args(d, 0, d.n_main_terms, d.n_terms, 0, slots, w->er, w->pt_tab);
        ma.skip = skip;
        if (!launch_msm_range(d, ma, n, w->scalars, w->pts, nullptr, pm, 1, SegBuf{w->msm_parts, w->shape.segs}))
            return fail(H2V_E_LIMIT, "internal: no MSM launch shape for this plan");
    }
    launch_pairing(d, n, w->pts, w->valid, w->valid_sub, w->er, nullptr, w->status, u.accept, nullptr, pm, w->in_flight_hint, skip);
    HIPCHK(hipGetLastError());
    if (u.status) HIPCHK(hipMemcpyAsync(u.status, w->status, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return H2V_OK;
}

// ---- the batch check over pairs (h2v_check_pairs_rlc; H2V_RLC_FOLD_PAIRS) ---------------------------------------------------
// u.n two-slot records of affine points in `pool` (the layout of w->pts).  Enqueues on `st`: the coefficient kernel
// (k_rlc_pairs_prepare), L = sum r_i L_i and R = sum r_i R_i as two bucket MSMs with 128-bit scalars in the same launches, ONE
// k_pairing_rlc over a one-proof view of the plan, and - skipped on the device when the check passed - the group stage.  The
// caller queues its stage 2 behind it with r->flags as skip flags.  good_given: r->good holds good_i already and `status` is
// final (k_fold_pairs_affine ran, behind the caller's ev[10]); otherwise valid / valid_sub of the two slots decide and
// H2V_ST_BAD_POINT is folded into `status`.  Events of the record: [10]/[4] around the coefficient kernel, [5] .. [8] the bucket
// MSMs, [8]/[9] around the pairing.  The workspace's failing-group estimate is not touched (stats = NULL).
static int pairs_rlc_core(const Unit &u, RlcWs *r, const uint32_t *pool, const uint8_t *valid, const uint8_t *valid_sub, bool good_given,
                          uint32_t *status, h2v_workspace *w, CallRec &rec, hipStream_t st) {
    const uint32_t n = u.n;
    hipEvent_t *ev = rec.ev;
    int rc;
    if (!good_given) HIPCHK(hipEventRecord(ev[10], st));
    RlcPairArgs ra = {n, status, valid, valid_sub, good_given ? r->good : nullptr, {}, r->r_scal, r->l_idx, r->r_idx, r->good, u.seed_dev, u.seed_xor7};
    copy_seed(ra.seed, u.seed);
    hipLaunchKernelGGL(k_rlc_pairs_prepare, dim3((n + 63) / 64), dim3(64), 0, st, ra);
    HIPCHK(hipEventRecord(ev[4], st));
    if ((rc = launch_sums(r, {n, 1, r->r_scal, r->r_idx, pool, 2 * n, nullptr}, {n, 1, r->r_scal, r->l_idx, pool, 2 * n, nullptr}, rec, st))) return rc;
    if (u.agg_parts) return agg_chunk(u, r, w, rec, st);      // (an aggregate call: the sums are exported, nothing is checked)
    if ((rc = launch_batch_pairing(u, r, grp_of_pairs(u.p, pool), nullptr, w, rec, st))) return rc;
    HIPCHK(hipGetLastError());
    return H2V_OK;
}
// One batch check over n encoded pairs: decoded as run_check decodes them (the same launch over the same two-slot view), then
// pairs_rlc_core; stage 2 of the fall-back is run_check's own pair of kernels on a walking grid behind the skip flags.
// Everything on `st`.  Events: [0]/[1] around the decoding, [2] = [3] (no transcript), then the core's.
static int run_pairs_rlc(const Unit &u, h2v_workspace *w, hipStream_t st) {
    const uint32_t n = u.n;
    LaunchOptsScope opts(w);
    int rc;
    if ((rc = pair_view_ensure(w)) || (rc = pair_rlc_ensure(w, false))) return rc;
    if (!u.fail_ctr && (rc = rlc_stats_ensure(w))) return rc;      // (the records' verdict words)
    const H2vDevPlan v = pair_view(u.p->d, w);
    RlcWs *r = w->prlc;
    CallRec &rec = rec_new(w, h2v_workspace::RLC);
    rec.no_vm = true;
    hipEvent_t *ev = rec.ev;
    for (int q : {0, 2, 3}) HIPCHK(hipEventRecord(ev[q], st));
    HIPCHK(hipMemsetAsync(w->status, 0, (size_t)n * 4, st));
    if ((rc = launch_decompress(v, n, u.pairs, w->pair_off, nullptr, nullptr, w, nullptr, st))) return rc;
    HIPCHK(hipEventRecord(ev[1], st));
    if ((rc = pairs_rlc_core(u, r, w->pts, w->valid, w->valid_sub, false, w->status, w, rec, st))) return rc;
    hipLaunchKernelGGL(k_pairs_to_jac, dim3((n + 63) / 64), dim3(64), 0, st, n, (const uint32_t *)w->pts, w->er, (const uint32_t *)r->flags);
    launch_pairing(v, n, w->pts, w->valid, w->valid_sub, w->er, nullptr, w->status, u.accept, nullptr, st, w->in_flight_hint, r->flags);
    HIPCHK(hipGetLastError());
    if (u.status) HIPCHK(hipMemcpyAsync(u.status, w->status, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return H2V_OK;
}
// H2V_RLC_FOLD_PAIRS: what run_pipeline enqueues in place of the per-proof pairing of a recursive plan.  After the fold every
// proof is a pair (el', er') like any other: k_fold_pairs_affine writes them into the set's pool, the core combines them, and
// the fall-back is the per-proof pairing on the folded points behind the skip flags - no MSM is repeated.
static int fold_pairs_tail(const Unit &u, const uint32_t *er2, const uint32_t *el2, h2v_workspace *w, CallRec &rec, hipStream_t st) {
    const uint32_t n = u.n;
    int rc;
    if ((rc = pair_rlc_ensure(w, true))) return rc;
    if (!u.fail_ctr && (rc = rlc_stats_ensure(w))) return rc;
    RlcWs *r = w->prlc;
    const H2vDevPlan &d = u.p->d;
    HIPCHK(hipEventRecord(rec.ev[10], st));
    hipLaunchKernelGGL(k_fold_pairs_affine, dim3((n + 63) / 64), dim3(64), 0, st, n, (uint32_t)H2V_SLOTS(d), w->valid, w->valid_sub, el2, er2, w->status, r->pool, r->good);
    if ((rc = pairs_rlc_core(u, r, r->pool, nullptr, nullptr, true, w->status, w, rec, st))) return rc;
    if (u.agg_parts) return H2V_OK;
    launch_pairing(d, n, w->pts, w->valid, w->valid_sub, er2, el2, w->status, u.accept, nullptr, st, w->in_flight_hint, r->flags);
    HIPCHK(hipGetLastError());
    return H2V_OK;
}
static bool fold_pairs_wanted(const h2v_plan *p, const h2v_rlc_opts *o) { return p->d.ivc && o && (o->flags & H2V_RLC_FOLD_PAIRS); }
// The batch coefficients must be unpredictable to whoever made the proofs: 32 bytes from the OS per call (getrandom; fails
// closed).  A caller-given seed (H2V_RLC_SEED_GIVEN) is for TESTS and reproducible measurements only; even then every call
// gets different coefficients - the process-wide call counter is mixed in - so that a service that copied a fixed seed
// from a test or from bench.py does not hand provers a combination they can cancel against... if they can predict the
// counter: a given seed is not a production setting.
#include <sys/random.h>
#include <atomic>
static int rlc_seed(const h2v_rlc_opts *o, uint32_t seed[8]) {
    if (o && (o->flags & H2V_RLC_SEED_GIVEN)) {
        static std::atomic<uint64_t> calls{0};
        const uint64_t k = calls.fetch_add(1);
        memcpy(seed, o->seed, 32);
        seed[5] ^= (uint32_t)k; seed[6] ^= (uint32_t)(k >> 32);
        return H2V_OK;
    }
    size_t got = 0;
    while (got < 32) {
        const ssize_t r = getrandom((uint8_t *)seed + got, 32 - got, 0);
        if (r <= 0) return fail(H2V_E_DEVICE, "no OS randomness for the batch coefficients (getrandom)");
        got += (size_t)r;
    }
    return H2V_OK;
}
#include "h2v_seed_host.hpp"   // derived seeds: the flags, seed_launch, seed_enqueue(_at), h2v_workspace_seed_used / _seed_ms
static int rlc_check_batch(const h2v_plan *p, const h2v_batch *b, const uint8_t *accept) {
    if (!p || !b || !accept) return fail(H2V_E_ARG, "null argument");
    if (b->n)
        if (int rc = batch_args(p, b)) return rc;
    if (b->n > (1ull << 22)) return fail(H2V_E_LIMIT, "RLC batches are limited to 2^22 proofs");
    return H2V_OK;
}
extern "C" int h2v_verify_batch_rlc_device(const h2v_plan *p, const h2v_batch *b, uint8_t *accept, uint32_t *status, h2v_workspace *ws,
                                           void *stream, const h2v_rlc_opts *opts) {
    int rc = rlc_check_batch(p, b, accept);
    if (rc) return rc;
    if (b->n == 0) return H2V_OK;
    if (!ws) return fail(H2V_E_ARG, "the RLC entry points need a workspace (results of the batch check live in it)");
    ALIVE(p); ALIVE(ws);
    HIPCHK(hipSetDevice(p->device));
    if ((rc = ws_fits(ws, p, b->n, false))) return rc;
    if (ws->pending) return fail(H2V_E_ARG, "the workspace has a host batch in flight: call h2v_verify_batch_wait first");
    if ((rc = null_stream_check(ws, stream))) return rc;
    // recursive plans fold an accumulator per proof (the challenge hashes that proof's own MSM result): no batch form, but
    // the opt-in one that starts after the fold
    Unit u = unit_of_batch(rlc_supported(p) ? UnitKind::RLC : fold_pairs_wanted(p, opts) ? UnitKind::FOLD_RLC : UnitKind::VERIFY, p, b, accept, status);
    u.one_stream_opt = opts && (opts->flags & H2V_RLC_ONE_STREAM);
    bool derive;
    if ((rc = seed_flags(opts, &derive))) return rc;
    u.derive = derive && u.batch_check();
    if (u.batch_check() && !u.derive && (rc = rlc_seed(opts, u.seed))) return rc;
    if (u.kind == UnitKind::RLC && !u.derive && co_wanted(ws, b->n)) return coalesce_call(u, ws, (hipStream_t)stream);   // (a derived seed is one call's)
    return run_call(u, ws, (hipStream_t)stream);
}
extern "C" int h2v_verify_batch_rlc(const h2v_plan *p, const h2v_batch *b, uint8_t *accept, h2v_workspace *ws, const h2v_rlc_opts *opts,
                                    int *fell_back) {
    int rc = rlc_check_batch(p, b, accept);
    if (rc) return rc;
    return verify_host(p, b, accept, ws, H2V_SUBMIT_RLC, opts, fell_back);
}

// ---- h2v_check_pairs_rlc(_device): h2v_check_pairs's contract, with ONE pairing for the batch when every pair's equation holds ----
static int pairs_rlc_args(const h2v_plan *p, uint64_t n, const uint8_t *pairs, const uint8_t *accept) {
    if (int rc = pairs_args(p, pairs, accept)) return rc;
    if (n > (1ull << 22)) return fail(H2V_E_LIMIT, "RLC batches are limited to 2^22 pairs");
    return H2V_OK;
}
extern "C" int h2v_check_pairs_rlc_device(const h2v_plan *p, uint64_t n, const uint8_t *pairs, uint8_t *accept, uint32_t *status,
                                          h2v_workspace *ws, void *stream, const h2v_rlc_opts *opts) {
    if (int rc = pairs_rlc_args(p, n, pairs, accept)) return rc;
    if (n == 0) return H2V_OK;
    if (!ws) return fail(H2V_E_ARG, "the RLC entry points need a workspace (results of the batch check live in it)");
    TmpWs none;
    if (int rc = pairs_common(p, n, ws, stream, true, none)) return rc;
    Unit u = unit_of_pairs(UnitKind::PAIR_RLC, p, n, pairs, accept, status);
    if (int rc = seed_flags(opts, &u.derive)) return rc;
    if (!u.derive)
        if (int rc = rlc_seed(opts, u.seed)) return rc;
    return run_call(u, ws, (hipStream_t)stream);
}
extern "C" int h2v_check_pairs_rlc(const h2v_plan *p, uint64_t n, const uint8_t *pairs, uint8_t *accept, uint32_t *status, h2v_workspace *ws,
                                   const h2v_rlc_opts *opts, int *fell_back) {
    if (int rc = pairs_rlc_args(p, n, pairs, accept)) return rc;
    if (fell_back) *fell_back = 0;
    if (n == 0) return H2V_OK;
    return check_pairs_host(Unit{UnitKind::PAIR_RLC, p, (uint32_t)n}, pairs, accept, status, ws, opts, fell_back);
}

#include "h2v_multi_srs.hpp"   // h2v_check_pairs_multi(_device): one batch check over pairs on several SRS
// ---------------------------------------------------------------------------------------------- mixed-key batches
// h2v_verify_mixed(_device): n proofs of SEVERAL plans on one SRS in one call.  Behind the per-proof MSM a proof of any key is a
// pair (L, R) with e(L, s_g2) == e(R, G2), and the pairing sees nothing of the key but the SRS; so the call runs
//   1. the partition (h2v_mixed.hpp, host) and k_mixed_gather: the proofs of each plan side by side in the workspace's staging;
//   2. per plan, the pipeline up to the pairing (MIXED_SUB units) - on a laned workspace the sub-batches of all plans
//      go round robin through the lanes and are in flight together;
//   3. ONE tail over the pool of pairs, which k_mixed_pairs filled in the CALLER's order: the per-proof pairing launch
//      (run_check's second half), or - H2V_MIXED_RLC - the batch check over pairs (pairs_rlc_core) with the per-pair kernels
//      behind its skip flags.  On a laned workspace the tail is cut into chunks like any check call, each its own batch check.
// The tables go up in one copy from a pinned block; a call takes one of four such blocks (and the device copy its kernels read),
// and a block is reused only when the call that took it last has finished on the device.
struct MixedWs {
    static constexpr int SLOTS = 4;
    struct Slot { Owner mem; uint8_t *h = nullptr, *d = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool used = false; } slot[SLOTS];
    Owner mem;                            // of the base buffers and the grouped staging (the slots, `in` and `fold` own theirs)
    uint64_t next = 0;
    int last = -1;                        // the slot of the most recent call: the next one starts behind its end, whatever its stream
    GrowBuf<false> proofs, inst, ci;                                 // grouped staging, grown on demand behind mixed_quiesce
    uint32_t *pool = nullptr, *status = nullptr;                     // the call's pairs (cap x 48 dwords) and status words, caller's order
    uint8_t *good = nullptr, *ones = nullptr;                        // good_i; 2 x cap bytes of 1: the `valid` of a two-slot view
    // host form: the staging slot of its own (stage_batch).  Not one of ws->hslot: a mixed call does not look at ws->pending, and
    // a submitted batch may be in flight in any of those
    h2v_workspace::HostSlot in;
    // H2V_MIXED_FOLD_MSM, allocated by the first fold call and grown behind mixed_quiesce: the call-level term pool - `fold` holds
    // the scalars of the R-terms (r_scal, fold_cap_terms records) and of the L-terms (l_scal, by call position), the per-block
    // sums of the VK-base scalars (vk_part, fold_cap_parts Fr records), good, the two bucket-MSM workspaces and the sums / misc /
    // flags set of the one pairing; fold_rpts / fold_lpts are the COPIED points of the terms (24 dwords each; fold's own blocks)
    struct RlcWs *fold = nullptr;
    uint32_t *fold_rpts = nullptr, *fold_lpts = nullptr;
    size_t fold_cap_terms = 0, fold_cap_parts = 0;
    bool fold_ran = false;                // fold->sums holds the sums of a fold call (h2v_probe_mixed_fold_sums)
    struct AcrossWs *across = nullptr;    // H2V_MIXED_ACROSS_SRS: the set of the one multi-pairing, created by the first such call
};
// one fold call: the pool, its layout, the device table of the foldable plans, the call's seed (ONE per call: chunks of a
// sub-batch do not derive their own, coefficients follow the position in the call)
// H2V_MIXED_GROUPED: which plans of a call are groupable and where their proofs lie among the grouped positions (decided on the
// host before anything is enqueued: mixed_group_layout), and - per range of a running call - the device tables of its groups
// (h2v_mixed_group.hpp), which travel in the call's pinned block
struct MixedGroupPlan {
    h2vmixed::GroupSpace sp;
    std::vector<h2vmixed::GroupShape> shapes;
};
struct MixedGroupRange : mixedtab::RangeInfo {     // the range's counts (h2v_mixed_tables.hpp) and its tables in the device block
    const H2vGroupRec *recs;
    const uint32_t *comb[2], *dec, *terms;
};
// ONE MIXED CALL: what it verifies, how, and where its results go.  Filled once by its entry point - mixed_args (plans, flags,
// partition), mixed_layouts, the seed, mixed_call_io (the I/O, and the one place where the combinations are checked) - and
// read-only from then on.  The second pass after a failed fold check is the same descriptor with fold and grouped cleared.
struct MixedCall {
    const h2v_plan *const *plans = nullptr;
    h2vmixed::Partition pt;
    bool rlc = false, fold = false, grouped = false;     // H2V_MIXED_RLC, _FOLD_MSM, _GROUPED
    bool across = false;                                 // H2V_MIXED_ACROSS_SRS: the tail cuts its left-hand sum by SRS class ...
    h2vsrs::Classes cls;                                 // ... these (mixed_args; h2v_mixed_srs.hpp)
    uint32_t seed[8] = {};                               // of the batch coefficients (rlc)
    // H2V_RLC_SEED_KEYED: the seed is derived from the call (form 3; mixed_seed) and `seed` stays zero.  plan_of: the caller's
    // (host memory in both forms), for the plan index of every leaf.  seed_prev: the second pass after a failed fold check - the
    // eight words the first pass derived, in the seed ring; nothing is hashed again
    bool keyed = false;
    const uint32_t *plan_of = nullptr;
    const uint32_t *seed_prev = nullptr;
    h2vmixed::FoldLayout lay;    // fold: the layout of the call's term pool (fold_layout over the workspace's chunk size)
    MixedGroupPlan grp;          // grouped: the groupable plans (lay's block sums then follow the grouped ranges)
    h2v_batch in = {};                                   // the call's device-resident buffers
    const uint64_t *host_off = nullptr;                  // the grouped proof offsets when the caller's proof_off is known on the host (the host form), else NULL
    uint8_t *accept = nullptr;
    uint32_t *status = nullptr;
    uint32_t *agg_parts = nullptr;                       // h2v_aggregate_mixed: the tail exports its sums to part 0, accept = included[]
};
struct MixedFold {
    MixedWs *m;
    const h2vmixed::FoldLayout *lay;
    const h2vmixed::Partition *pt;
    const h2v_plan *const *plans;
    const H2vFoldPlan *d_plans;           // lay->n_foldable entries
    const uint32_t *d_perm;               // grouped index -> position in the call
    uint32_t seed[8];
    const uint32_t *seed_dev = nullptr;   // H2V_RLC_SEED_KEYED: the call's slot of the seed ring, read in place of `seed`
    const MixedGroupPlan *grp = nullptr;  // H2V_MIXED_GROUPED
    std::vector<MixedGroupRange> ranges;  // its ranges, in order
    const uint64_t *d_off = nullptr;      // the grouped proof offsets (n + 1)
    const h2vsrs::Classes *cls = nullptr; // H2V_MIXED_ACROSS_SRS: the call's SRS classes ...
    const uint32_t *d_cpos = nullptr;     // ... and their position list on the device: class-major slot -> call position (n)
};
static void across_release(MixedWs *m);
static int across_fold_sums(const Unit &u, h2v_workspace *w, CallRec &rec, hipStream_t st);
static void across_fold_reset(MixedWs *m);
static void mixed_release(h2v_workspace *w) {
    MixedWs *m = w->mixed;
    if (!m) return;
    for (auto &s : m->slot)
        if (s.used && s.done) (void)hipEventSynchronize(s.done);
    for (auto &s : m->slot) s.mem.release();
    slot_release(m->in);
    if (m->fold) rlc_release(m->fold);
    across_release(m);
    m->mem.release();
    delete m;
    w->mixed = nullptr;
}
// every earlier mixed call on w has finished on the device (before staging is freed or re-allocated)
static int mixed_quiesce(MixedWs *m) {
    for (auto &s : m->slot)
        if (s.used) { HIPCHK(hipEventSynchronize(s.done)); s.used = false; }
    return H2V_OK;
}
static int mixed_ensure(h2v_workspace *w, const h2vmixed::Partition &pt) {
    if (!w->mixed) {
        MixedWs *m = new MixedWs();
        w->mixed = m;
        const auto T = wslayout::mixed_base(w->cap);
        bool ok = m->mem.alloc(m->pool, T.row[wslayout::M_POOL]) && m->mem.alloc(m->status, T.row[wslayout::M_STATUS]) &&
                  m->mem.alloc(m->good, T.row[wslayout::M_GOOD]) && m->mem.alloc(m->ones, T.row[wslayout::M_ONES]);
        for (auto &s : m->slot) ok = ok && s.mem.event(s.done, hipEventDisableTiming);
        if (!ok) { mixed_release(w); return fail(H2V_E_DEVICE, "allocation of the mixed-call buffers failed"); }
    }
    MixedWs *m = w->mixed;
    auto quiet = [m]() { return mixed_quiesce(m); };
    if (int rc = m->proofs.ensure(m->mem, (size_t)pt.proof_cap + 64, "the mixed-call staging", quiet)) return rc;
    if (int rc = m->inst.ensure(m->mem, (size_t)pt.inst_total + 64, "the mixed-call staging", quiet)) return rc;
    return m->ci.ensure(m->mem, (size_t)pt.ci_total * 48 + 64, "the mixed-call staging", quiet);
}
// The term pool of the fold form for a call of this layout (the first fold call allocates, a larger one grows it once every
// earlier mixed call has finished on the device).
static int mixed_fold_ensure(h2v_workspace *w, const h2vmixed::FoldLayout &lay) {
    MixedWs *m = w->mixed;
    const size_t need_t = (size_t)lay.n_r, need_p = (size_t)lay.n_parts;
    if (m->fold && need_t <= m->fold_cap_terms && need_p <= m->fold_cap_parts) return H2V_OK;
    if (int rc = mixed_quiesce(m)) return rc;
    if (m->fold) { rlc_release(m->fold); m->fold = nullptr; }
    m->fold_rpts = m->fold_lpts = nullptr;
    const wslayout::FoldCaps caps = wslayout::fold_caps(need_t, need_p, m->fold_cap_terms, m->fold_cap_parts);
    const size_t cap_t = caps.terms, cap_p = caps.parts;
    m->fold_cap_terms = m->fold_cap_parts = 0; m->fold_ran = false;
    RlcWs *r = rlc_new(w->cap, 0, 0, wslayout::rlc_fold(w->cap, cap_t, cap_p));
    if (!r) return fail(H2V_E_DEVICE, "allocation of the fold form's term pool failed");
    m->fold_rpts = r->fold_rpts; m->fold_lpts = r->fold_lpts;
    m->fold = r; m->fold_cap_terms = cap_t; m->fold_cap_parts = cap_p;
    return H2V_OK;
}
// H2V_MIXED_FOLD_MSM, a sub-batch (or a lane's chunk of one) of a plan that has the batch form: phase 1 exactly as run_rlc runs it
// - the decompression launch builds no window tables, the combiner beside it, joined - and then k_mixed_terms: the proofs'
// scaled scalars and COPIES of their points into the call's term pool, their share of the VK-base sums, and good / status /
// (r, pi) at their positions in the call.  No MSM, no pair, no pairing.  The record is a prepare call's; events as run_pipeline's:
// [0]/[1] around the combiner, [2]/[3] around the decompression, [4] = [5] (no MSM), [5]/[6] around k_mixed_terms.
static int run_mixed_terms(const Unit &u, h2v_workspace *w, hipStream_t st) {
    const h2v_plan *p = u.p;
    const H2vDevPlan &d = p->d;
    const MixedFold &f = *u.fold;
    const h2vmixed::FoldLayout &lay = *f.lay;
    const uint32_t n = u.n, k = u.fold_plan, slots = H2V_SLOTS(d);
    LaunchOptsScope opts(w);
    int rc;
    CallRec &rec = rec_new(w, h2v_workspace::PREPARE);
    hipEvent_t *ev = rec.ev;
    const bool one_stream = w->one_stream_mode >= 0 ? w->one_stream_mode == 1 : w->in_flight_hint >= 3;
    hipStream_t pm = st;
    rc = phase1(w, st, one_stream, ev + 2, ev + 0,
                [&](hipStream_t ps) { return launch_decompress(d, n, u.proofs, u.off, u.ci, u.inst, w, nullptr, ps); },
                [&](hipStream_t s) { return launch_vm(d, n, w->stride, u.proofs, u.off, u.inst, u.ci, w->regs, w->scalars, w->status, nullptr, s); });
    if (rc) return rc;
    HIPCHK(hipEventRecord(ev[4], pm));
    HIPCHK(hipEventRecord(ev[5], pm));
    RlcWs *r = f.m->fold;
    const size_t t0 = (size_t)lay.term_base[k] + (size_t)u.first * p->n_var;                                   // the chunk's first R-term
    const size_t b0 = (size_t)lay.part_base[k] + (size_t)h2vmixed::fold_chunk_block(u.first, lay.chunk) * p->n_fix;   // ... and Fr record
    if (t0 + (size_t)n * p->n_var > f.m->fold_cap_terms || b0 + (size_t)((n + 63) / 64) * p->n_fix > f.m->fold_cap_parts)
        return fail(H2V_E_DEVICE, "internal: a chunk's terms lie outside the call's term pool");
    MixedTermsArgs a = {n, p->n_var, p->n_fix, slots, d.pi_point, d.n_terms, d.terms, w->scalars, w->status, w->valid, w->valid_sub, w->pts, u.pos, {},
                        r->r_scal + t0 * 8, f.m->fold_rpts + t0 * 24, r->l_scal, f.m->fold_lpts, r->vk_part + b0 * 8, u.pool.good, u.pool.status};
    copy_seed(a.seed, f.seed);
    a.seed_dev = f.seed_dev;
    hipLaunchKernelGGL(k_mixed_terms, dim3((n + 63) / 64), dim3(64), 0, pm, a);
    HIPCHK(hipEventRecord(ev[6], pm));
    HIPCHK(hipGetLastError());
    return H2V_OK;
}
// H2V_MIXED_GROUPED, one range of the grouped positions (u.first .. + u.n): run_mixed_terms for every groupable plan's share of
// the range at once - ONE decompression launch without window tables, the combiner beside it (one launch per transcript kind that
// has proofs in the range), joined, then ONE k_mixed_terms_grouped.  Every block finds its plan in the range's group table; every
// plan runs its narrow schedule with P = vm_lds_slots (the workspace's combiner options shape per-plan launches only).  Group g's
// sub-batch lies at its first position x the call's union strides in the workspace's buffers.  The record is a prepare call's;
// events [0]/[1] around the combiner launches, [2]/[3] around the decompression, [4]/[5] around k_mixed_terms_grouped (so that
// h2v_workspace_timings reports it where a pipeline reports its MSM), [6] = [5].
static int run_mixed_group(const Unit &u, h2v_workspace *w, hipStream_t st) {
    const MixedFold &f = *u.fold;
    const h2vmixed::GroupSpace &sp = f.grp->sp;
    const size_t c = sp.chunk ? u.first / sp.chunk : 0u;
    if (c >= f.ranges.size() || f.ranges[c].n != u.n || (sp.chunk && u.first % sp.chunk))
        return fail(H2V_E_DEVICE, "internal: a grouped unit is not a range of the call");
    const MixedGroupRange &g = f.ranges[c];
    if (u.n > w->cap || sp.u_terms > w->shape.terms || sp.u_slots > w->shape.slots)
        return fail(H2V_E_DEVICE, "internal: a grouped range does not fit the workspace");
    LaunchOptsScope opts(w);
    int rc;
    CallRec &rec = rec_new(w, h2v_workspace::PREPARE);
    hipEvent_t *ev = rec.ev;
    const bool one_stream = w->one_stream_mode >= 0 ? w->one_stream_mode == 1 : w->in_flight_hint >= 3;
    hipStream_t pm = st;
    MixedWs *m = f.m;
    auto decompress = [&](hipStream_t ps) -> int {
        const uint32_t units = 2 * g.units, max_blocks = (uint32_t)(msm_n_simd() / 4.0);
        const uint32_t blocks = (units + 3) / 4 < max_blocks ? (units + 3) / 4 : max_blocks;
        HIPCHK(hipMemsetAsync(w->dec_ctr, 0, 4, ps));
        const GroupDecompressArgs da = {g.recs, g.dec, g.n_groups, g.units, m->proofs.p, f.d_off, m->inst.p, m->ci.p, w->pts, w->valid, w->valid_sub, w->dec_ctr};
        hipLaunchKernelGGL(k_g1_decompress_queue_grouped, dim3(blocks), dim3(256), 0, ps, da);
        return H2V_OK;
    };
    auto combine = [&](hipStream_t s) -> int {      // one launch per transcript kind that has proofs in the range
        for (int t = 0; t < 2; t++) {
            if (!g.blocks_comb[t]) continue;
            const auto k_grp = t == (int)H2V_TR_BLAKE2B_512 ? k_transcript_combiner_grouped_b512 : k_transcript_combiner_grouped;
            if (g.lds[t] > H2V_VM_LDS_BYTES) return fail(H2V_E_DEVICE, "internal: a grouped plan's register file does not fit LDS");
            HIPCHK(hipFuncSetAttribute((const void *)k_grp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds[t]));
            const GroupCombinerArgs ca = {g.recs, g.comb[t], g.n_groups, m->proofs.p, f.d_off, m->inst.p, m->ci.p, w->scalars, (uint32_t *)w->status};
            hipLaunchKernelGGL(k_grp, dim3(g.blocks_comb[t]), dim3(64), g.lds[t], s, ca);
        }
        return H2V_OK;
    };
    if ((rc = phase1(w, st, one_stream, ev + 2, ev + 0, decompress, combine))) return rc;
    HIPCHK(hipEventRecord(ev[4], pm));
    RlcWs *r = m->fold;
    GroupTermsArgs ta = {g.recs, g.terms, g.n_groups, w->scalars, (const uint32_t *)w->status, w->valid, w->valid_sub, w->pts, f.d_perm, {},
                         r->r_scal, m->fold_rpts, r->l_scal, m->fold_lpts, r->vk_part, u.pool.good, u.pool.status};
    copy_seed(ta.seed, f.seed);
    ta.seed_dev = f.seed_dev;
    hipLaunchKernelGGL(k_mixed_terms_grouped, dim3(g.blocks_terms), dim3(64), 0, pm, ta);
    HIPCHK(hipEventRecord(ev[5], pm));
    HIPCHK(hipEventRecord(ev[6], pm));
    HIPCHK(hipGetLastError());
    return H2V_OK;
}
// H2V_MIXED_FOLD_MSM, the tail, behind every sub-batch of the call: the VK-base terms of the foldable plans (k_mixed_vk_sum), one
// pair of terms per proof of the other plans out of the call's pool of pairs (k_mixed_pair_terms), then R over the term pool
// (255-bit scalars, GLV) and L over the n call positions (128-bit) side by side in the six bucket-MSM launches, and ONE
// k_pairing_rlc without a group stage, whose epilogue writes accept[i] = good_i in the caller's order when the check passes.  A
// failed check leaves accept[] alone: the host runs the H2V_MIXED_RLC path then (run_mixed_call).  w: the ordinary workspace, or
// the lane whose record the tail takes - none of its buffers is used.  Events as run_pairs_rlc's (no decoding, no transcript).
static int run_mixed_fold_tail(const Unit &u, h2v_workspace *w, hipStream_t st) {
    const MixedFold &f = *u.fold;
    const h2vmixed::FoldLayout &lay = *f.lay;
    MixedWs *m = f.m;
    RlcWs *r = m->fold;
    const uint32_t n = u.n;
    LaunchOptsScope opts(w);
    int rc;
    if (!u.fail_ctr && (rc = rlc_stats_ensure(w))) return rc;
    CallRec &rec = rec_new(w, h2v_workspace::RLC);
    rec.no_vm = true;
    for (int q : {0, 1, 2, 3, 10}) HIPCHK(hipEventRecord(rec.ev[q], st));
    HIPCHK(hipMemcpyAsync(r->good, m->good, n, hipMemcpyDeviceToDevice, st));
    if (lay.total_fix)
        hipLaunchKernelGGL(k_mixed_vk_sum, dim3((lay.total_fix + 63) / 64), dim3(64), 0, st, f.d_plans, lay.n_foldable, lay.total_fix, (const uint32_t *)r->vk_part,
                           r->r_scal, m->fold_rpts);
    for (uint32_t k = 0; k < lay.n_plans; k++) {
        if (!f.pt->count[k] || lay.foldable[k]) continue;
        MixedPairTermsArgs pa = {f.pt->count[k], lay.pair_base[k], f.d_perm + f.pt->base[k], m->pool, m->good, {}, r->r_scal, m->fold_rpts, r->l_scal, m->fold_lpts};
        copy_seed(pa.seed, f.seed);
        pa.seed_dev = f.seed_dev;
        hipLaunchKernelGGL(k_mixed_pair_terms, dim3((pa.n + 63) / 64), dim3(64), 0, st, pa);
    }
    if (f.cls) return across_fold_sums(u, w, rec, st);      // (H2V_MIXED_ACROSS_SRS: h2v_mixed_across.hpp)
    HIPCHK(hipEventRecord(rec.ev[4], st));
    if ((rc = launch_sums(r, {(uint32_t)lay.n_r, 2, r->r_scal, nullptr, m->fold_rpts, (uint32_t)lay.n_r, nullptr}, {n, 1, r->l_scal, nullptr, m->fold_lpts, n, nullptr}, rec, st))) return rc;
    if (u.agg_parts) rc = agg_chunk(u, r, w, rec, st);
    else rc = launch_batch_pairing(u, r, GrpShape{}, nullptr, w, rec, st, false);
    if (rc) return rc;
    m->fold_ran = true;
    across_fold_reset(m);      // (the most recent fold call is on one SRS)
    HIPCHK(hipGetLastError());
    if (u.status) HIPCHK(hipMemcpyAsync(u.status, m->status, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return H2V_OK;
}
// The tail over u.n pairs of the pool (two-slot affine records, caller's order) on an ordinary workspace or a lane: the per-proof
// pairing launch of run_check, or (MIXED_TAIL_RLC) the batch check of run_pairs_rlc, both without their decoding - the pipeline
// made these points itself.  Events as run_check's / run_pairs_rlc's.
static int run_mixed_tail(const Unit &u, h2v_workspace *w, hipStream_t st) {
    const uint32_t m = u.n;
    const MixedPool &mp = u.pool;
    LaunchOptsScope opts(w);
    int rc;
    if ((rc = pair_view_ensure(w))) return rc;
    const H2vDevPlan v = pair_view(u.p->d, w);
    if (u.kind == UnitKind::MIXED_TAIL) {
        CallRec &rec = rec_new(w, h2v_workspace::CHECK);
        hipEvent_t *ev = rec.ev;
        for (int q : {0, 1, 2, 3, 4}) HIPCHK(hipEventRecord(ev[q], st));
        hipLaunchKernelGGL(k_pairs_to_jac, dim3((m + 63) / 64), dim3(64), 0, st, m, (const uint32_t *)mp.pool, w->er, (const uint32_t *)nullptr);
        HIPCHK(hipEventRecord(ev[5], st));
        rec.pair = (uint8_t)launch_pairing(v, m, mp.pool, mp.ones, nullptr, w->er, nullptr, mp.status, u.accept, nullptr, st, w->in_flight_hint);
        HIPCHK(hipEventRecord(ev[6], st));
    } else {
        if ((rc = pair_rlc_ensure(w, false))) return rc;
        if (!u.fail_ctr && (rc = rlc_stats_ensure(w))) return rc;
        RlcWs *r = w->prlc;
        CallRec &rec = rec_new(w, h2v_workspace::RLC);
        rec.no_vm = true;
        for (int q : {0, 1, 2, 3, 10}) HIPCHK(hipEventRecord(rec.ev[q], st));
        HIPCHK(hipMemcpyAsync(r->good, mp.good, m, hipMemcpyDeviceToDevice, st));
        if ((rc = pairs_rlc_core(u, r, mp.pool, nullptr, nullptr, true, mp.status, w, rec, st))) return rc;
        hipLaunchKernelGGL(k_pairs_to_jac, dim3((m + 63) / 64), dim3(64), 0, st, m, (const uint32_t *)mp.pool, w->er, (const uint32_t *)r->flags);
        launch_pairing(v, m, mp.pool, mp.ones, nullptr, w->er, nullptr, mp.status, u.accept, nullptr, st, w->in_flight_hint, r->flags);
    }
    HIPCHK(hipGetLastError());
    if (u.status) HIPCHK(hipMemcpyAsync(u.status, mp.status, (size_t)m * 4, hipMemcpyDeviceToDevice, st));
    return H2V_OK;
}
#include "h2v_mixed_across.hpp"   // H2V_MIXED_ACROSS_SRS: the set of the one multi-pairing and the two tails that end in it
// ---- run_mixed in parts: the tables, the units, the two schedules
// The next of the four table blocks, once the call that took it last has finished on the device (its copy and its kernels are
// done), grown to `need` bytes.
static int mixed_slot(MixedWs *m, size_t need, int *si) {
    *si = (int)(m->next++ % MixedWs::SLOTS);
    MixedWs::Slot &sl = m->slot[*si];
    if (sl.used) { HIPCHK(hipEventSynchronize(sl.done)); sl.used = false; }
    if (need <= sl.cap) return H2V_OK;
    sl.mem.drop(sl.h); sl.mem.drop(sl.d);
    sl.cap = 0;
    const size_t cap = wslayout::grown(need);
    if (!sl.mem.alloc_pinned(sl.h, cap) || !sl.mem.alloc(sl.d, cap))
        return fail(H2V_E_DEVICE, "allocation of the mixed-call tables failed");
    sl.cap = cap;
    return H2V_OK;
}
// THE TABLES of a call: one pinned block (h2v_mixed_tables.hpp lays it out and packs it), one copy on `st` behind the last call's
// block - the staging is that call's until then.  On success the block is IN USE: whoever called records sl->done behind the call.
struct MixedTables {
    MixedWs::Slot *sl = nullptr;
    uint64_t *d_off = nullptr;                // the grouped proof offsets (n + 1)
    H2vMixedTab tab = {};
    const H2vFoldPlan *d_fold = nullptr;      // fold: lay.n_foldable entries
    std::vector<MixedGroupRange> ranges;      // grouped: its ranges, in order
    const uint32_t *d_plan_idx = nullptr, *d_key_tags = nullptr;      // keyed leaves: the plan of every grouped position; 8 dwords per listed plan
    const uint32_t *d_cpos = nullptr;         // across SRS: class-major slot -> call position (n)
};
static int mixed_tables(const MixedCall &c, h2v_workspace *w, hipStream_t st, MixedTables &out) {
    MixedWs *m = w->mixed;
    const h2vmixed::Partition &pt = c.pt;
    std::vector<h2vmixed::GroupTables> gt(c.grouped ? h2vmixed::group_ranges(c.grp.sp) : 0u);
    std::vector<uint32_t> n_groups(gt.size());
    for (size_t q = 0; q < gt.size(); q++) {
        uint32_t g0, g1;
        h2vmixed::group_range(c.grp.sp, (uint32_t)q, g0, g1);
        std::string err;
        if (!h2vmixed::group_tables(c.grp.sp, c.grp.shapes.data(), pt, c.lay, g0, g1, m->fold_cap_terms, m->fold_cap_parts, gt[q], &err)) return fail(H2V_E_DEVICE, err);
        n_groups[q] = (uint32_t)gt[q].rec.size();
    }
    const bool leaves = c.keyed && !c.seed_prev;      // (the pass that derives: the second pass of a call copies eight words)
    const mixedtab::TableBlock B = mixedtab::table_block(pt.n, c.fold ? (size_t)c.lay.n_foldable * sizeof(H2vFoldPlan) : 0, n_groups.data(), n_groups.size(),
                                                         leaves ? pt.n_plans : 0u, c.across);
    int si;
    if (int rc = mixed_slot(m, B.extent, &si)) return rc;
    MixedWs::Slot &sl = m->slot[si];
    std::vector<mixedtab::RangeInfo> info;
    std::vector<uint8_t> tags(leaves ? (size_t)pt.n_plans * 32 : 0u);
    for (uint32_t k = 0; leaves && k < pt.n_plans; k++) memcpy(tags.data() + (size_t)k * 32, c.plans[k]->key_tag, 32);
    mixedtab::pack_tables(sl.h, B, pt, c.host_off, gt, info, leaves ? c.plan_of : nullptr, leaves ? tags.data() : nullptr);
    if (c.across) memcpy(sl.h + B.class_pos.off, c.cls.pos.data(), B.class_pos.bytes);      // (h2v_mixed_srs.hpp: slot -> call position)
    if (c.fold) {            // what k_mixed_vk_sum reads of the foldable plans, in list order (device pointers: written here)
        H2vFoldPlan *fp = (H2vFoldPlan *)(sl.h + B.fold.off);
        for (uint32_t k = 0; k < pt.n_plans; k++)
            if (c.lay.foldable[k])
                *fp++ = H2vFoldPlan{c.plans[k]->d.vk_bases, c.plans[k]->d.terms, c.plans[k]->n_var, c.plans[k]->n_fix, c.lay.fix_base[k], c.lay.n_blocks[k], c.lay.vk_base[k], 0u, c.lay.part_base[k]};    }
    if (m->last >= 0 && m->last != si && m->slot[m->last].used) HIPCHK(hipStreamWaitEvent(st, m->slot[m->last].done, 0));
    HIPCHK(hipMemcpyAsync(sl.d, sl.h, B.extent, hipMemcpyHostToDevice, st));
    sl.used = true; m->last = si;
    auto dev = [&sl](const mixedtab::Region &g) { return sl.d + g.off; };
    out.sl = &sl;
    out.d_off = (uint64_t *)dev(B.offsets);
    out.tab = {pt.n, (const uint64_t *)dev(B.inst_src), (const uint64_t *)dev(B.inst_dst), (const uint32_t *)dev(B.perm), (const uint32_t *)dev(B.len_cap),
               (const uint32_t *)dev(B.inst_len), (const uint32_t *)dev(B.ci_src), (const uint32_t *)dev(B.ci_dst)};
    out.d_fold = (const H2vFoldPlan *)dev(B.fold);
    out.d_plan_idx = (const uint32_t *)dev(B.plan_idx); out.d_key_tags = (const uint32_t *)dev(B.key_tags);
    out.d_cpos = c.across ? (const uint32_t *)dev(B.class_pos) : nullptr;
    out.ranges.resize(gt.size());
    for (size_t q = 0; q < gt.size(); q++) {
        MixedGroupRange &r = out.ranges[q];
        const mixedtab::RangeRegions &g = B.range[q];
        static_cast<mixedtab::RangeInfo &>(r) = info[q];
        r.recs = (const H2vGroupRec *)dev(g.recs); r.dec = (const uint32_t *)dev(g.dec); r.terms = (const uint32_t *)dev(g.terms);
        for (int t = 0; t < 2; t++) r.comb[t] = (const uint32_t *)dev(g.comb[t]);
    }
    return H2V_OK;
}
// THE UNITS of a call.  phase1: the grouped unit if the call has grouped positions, then the sub-batch of every plan that runs one
// of its own - every plan with proofs, but for the groupable ones of a grouped call, which share that ONE unit and one record -
// in list order: the records the call takes before its tail's.  tail: over the whole pool.  The units point at `fc`.
struct MixedUnits {
    MixedFold fc;
    std::vector<Unit> phase1;
    Unit tail = {};
    MixedUnits() = default;
    MixedUnits(const MixedUnits &) = delete;
};
static void mixed_units(const MixedCall &c, MixedTables &t, MixedWs *m, MixedUnits &mu) {
    const h2vmixed::Partition &pt = c.pt;
    const MixedPool pool = {m->pool, m->good, m->ones, m->status};
    MixedFold &fc = mu.fc;
    fc.m = m; fc.lay = c.fold ? &c.lay : nullptr; fc.pt = &pt; fc.plans = c.plans; fc.d_plans = t.d_fold; fc.d_perm = t.tab.perm;
    copy_seed(fc.seed, c.seed);
    fc.grp = c.grouped ? &c.grp : nullptr; fc.ranges = std::move(t.ranges); fc.d_off = t.d_off;
    fc.cls = c.across ? &c.cls : nullptr; fc.d_cpos = t.d_cpos;
    const uint32_t G = c.grouped ? c.grp.sp.total : 0u;
    if (G) {
        Unit group{UnitKind::MIXED_GROUP, nullptr, G};
        group.fold = &fc; group.pool = pool;
        mu.phase1.push_back(group);
    }
    const h2v_plan *p0 = nullptr;          // any plan of the call: the tail reads nothing of it but the SRS's line tables
    for (uint32_t k = 0; k < pt.n_plans; k++) {
        if (!pt.count[k]) continue;                                  // (a listed plan without a proof costs nothing)
        if (!p0) p0 = c.plans[k];
        if (c.grouped && c.grp.sp.groupable[k]) continue;
        // plan k's sub-batch out of the grouped staging
        const H2vDevPlan &d = c.plans[k]->d;
        Unit u{c.fold && c.lay.foldable[k] ? UnitKind::MIXED_SUB_TERMS : UnitKind::MIXED_SUB, c.plans[k], pt.count[k]};
        if (c.fold) { u.fold = &fc; u.fold_plan = k; }
        u.proofs = m->proofs.p; u.off = t.d_off + pt.base[k];
        u.inst = d.n_pi ? m->inst.p + pt.inst_base[k] : nullptr;
        u.ci = d.n_ci ? m->ci.p + (size_t)pt.ci_base[k] * 48 : nullptr;
        u.pos = t.tab.perm + pt.base[k]; u.pool = pool;
        mu.phase1.push_back(u);
    }
    if (G) mu.phase1.front().p = p0;
    mu.tail = Unit{c.fold ? UnitKind::MIXED_FOLD_TAIL : c.across ? UnitKind::MIXED_ACROSS_TAIL : c.rlc ? UnitKind::MIXED_TAIL_RLC : UnitKind::MIXED_TAIL, p0, pt.n};
    mu.tail.pool = pool; mu.tail.accept = c.accept; mu.tail.status = c.status;
    if (c.fold) { mu.tail.fold = &fc; mu.tail.agg_parts = c.agg_parts; }
    if (c.across) mu.tail.fold = &fc;      // (the classes and their position list)
    copy_seed(mu.tail.seed, c.seed);
}
// an ordinary workspace: the sub-batches one after the other on `st`, then the tail (one stream: everything is joined by
// construction)
static int mixed_run_ordinary(const MixedUnits &mu, h2v_workspace *w, hipStream_t st) {
    for (const Unit &u : mu.phase1)
        if (int rc = run_unit(u, w, st)) return rc;
    return run_unit(mu.tail, w, st);
}
// a laned workspace: every phase-1 unit in chunks through the lanes, nothing joined in between; then the tail behind all of them.
// More than RING records in one pass (the second pass of a grouped call of more than 64 plans with proofs): the sub-batches run
// in slices of at most SLICE plans, every slice joined before the next one starts, so that no record's slot is taken again while
// its kernels are in flight; the ONE tail stays the call's last record.  (The grouped unit is no member of a slice.)
static int mixed_run_laned(const MixedCall &c, MixedUnits &mu, h2v_workspace *w, hipStream_t st) {
    constexpr uint32_t SLICE = 62;
    const uint32_t n = c.pt.n, used_plans = (uint32_t)mu.phase1.size();
    const bool sliced = used_plans > H2V_MIXED_MAX_PLANS, rlc = c.rlc;
    Unit &tail = mu.tail;
    int rc;
    uint32_t total_chunks = 0;
    for (const Unit &u : mu.phase1) total_chunks += n_chunks(u.n, w->chunk);
    // (the sub-batches of all plans are in flight together: what they may assume is the call's chunks, not one plan's)
    const uint32_t sub_hint = call_hint(w, total_chunks > w->n_lanes, total_chunks);
    tail.fail_ctr = w->rec_fail ? w->rec_fail + (w->calls + used_plans) % h2v_workspace::RING : nullptr;   // the tail's record: the call's last
    if (rlc && !tail.fail_ctr) return fail(H2V_E_DEVICE, "internal: no verdict words");
    if (rlc && hipMemsetAsync(tail.fail_ctr, 0, 4, st) != hipSuccess) return fail(H2V_E_DEVICE, "memset failed");
    if (hipEventRecord(w->ev_fork, st) != hipSuccess) return fail(H2V_E_DEVICE, "event record failed");
    bool used_lane[h2v_workspace::MAXL] = {};
    uint32_t in_slice = 0;
    for (const Unit &u : mu.phase1) {
        if (sliced && u.kind != UnitKind::MIXED_GROUP && in_slice++ == SLICE) {   // the next slice starts behind the whole of this one
            if ((rc = lanes_join(w, st))) return rc;
            if (hipEventRecord(w->ev_fork, st) != hipSuccess) return fail(H2V_E_DEVICE, "event record failed");
            in_slice = 1;
        }
        int stream_mode = 1;
        const uint32_t L = laned_depth(w, u.n, false, &stream_mode);
        rec_laned(w, h2v_workspace::PREPARE, L, u.n, w->chunk);
        if ((rc = run_chunks(w, u, L, w->chunk, {sub_hint, stream_mode}, [&](uint32_t l, hipStream_t) { used_lane[l] = true; return (int)H2V_OK; }))) return rc;
    }
    if (c.fold || c.across) {
        // ---- the fold form's tail, and the tail of a call across several SRS: ONE piece on the call's stream, behind every lane;
        // its record (one "chunk") is a lane's
        if ((rc = lanes_join(w, st))) return rc;
        CallRec &rec = rec_laned(w, h2v_workspace::RLC, w->n_lanes, n, n);
        rec.agg = tail.agg_parts != nullptr;
        if (rec_word(w, rec) != tail.fail_ctr) return fail(H2V_E_DEVICE, "internal: the tail's record is not the call's last");
        const uint32_t l = (uint32_t)(w->next_lane++ % w->n_lanes);
        if ((rc = ensure_lane(w, l))) return rc;
        return run_unit(tail, w->lane[l], st);
    }
    // ---- the tail: chunks of the pool in the caller's order, each behind EVERY sub-batch (any of them may hold any position)
    const uint32_t L = laned_depth(w, n, rlc, nullptr), nch = n_chunks(n, w->chunk);
    rec_laned(w, rlc ? h2v_workspace::RLC : h2v_workspace::CHECK, L, n, w->chunk);
    auto behind_subs = [&](uint32_t l, hipStream_t ls) -> int {
        for (uint32_t q = 0; q < w->n_lanes; q++)
            if (used_lane[q] && q != l && hipStreamWaitEvent(ls, w->lane_ev[q], 0) != hipSuccess) return fail(H2V_E_DEVICE, "stream wait failed");
        used_lane[l] = true;
        return H2V_OK;
    };
    // (a mixed call joins at its end: its tail has only its own chunks in flight unless joins are deferred)
    if ((rc = run_chunks(w, tail, L, w->chunk, {call_hint(w, false, nch < L ? nch : L), 1}, behind_subs))) return rc;
    // a mixed call is a join point: its caller-stream wait happens here, deferred joins or not
    return lanes_join(w, st);
}
// H2V_RLC_SEED_KEYED, THE place where a mixed call gets its seed: on the call's stream behind the table upload (and so behind the
// host form's input upload) and in front of everything the pass forks to lanes or sub-batches.  The slot of the seed ring is the
// one of the pass's LAST record - the tail's, `records` - 1 records ahead -, chosen before any record is taken: every consumer of the
// pass reads that slot, h2v_workspace_seed_used / _seed_ms find it through the call's last record, and no other record of the
// call is ever handed it, because records do not write the ring - only a derivation does, and a call has one.  The first pass
// derives (seed_enqueue_at: the ring, the digest buffer and the events are seed_enqueue's); the second pass of a fold call that
// failed its check (c.seed_prev) copies the eight words to its own tail's slot - the first pass has finished, the stream was
// synchronised for its verdict - and takes over the two timed events of the derivation, so that the getters answer for the
// call's last record whether it fell back or not.  The digest kernels read the CALLER's buffers (c.in): proofs as given.
static int mixed_seed(const MixedCall &c, const MixedTables &t, h2v_workspace *w, hipStream_t st, size_t records, const uint32_t **seed_dev) {
    constexpr uint32_t RING = h2v_workspace::RING;
    const uint32_t slot = (uint32_t)((w->calls + records - 1) % RING);
    if (!c.seed_prev) {
        const SeedMixedLeafArgs ma = {c.pt.n, t.tab.perm, t.tab.inst_src, t.tab.inst_len, t.tab.ci_src, t.d_plan_idx, t.d_key_tags,
                                      c.in.proofs, c.in.proof_off, c.in.instances, c.in.committed, {}, nullptr};
        SeedJob j = {h2vseed::FORM_MIXED, c.pt.n, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        j.mixed = &ma;
        return seed_enqueue_at(w, st, slot, j, seed_dev);
    }
    uint32_t *const dst = w->seed_ring + (size_t)slot * 8;
    const size_t from = (size_t)(c.seed_prev - w->seed_ring) / 8;
    if (dst != c.seed_prev) {
        HIPCHK(hipMemcpyAsync(dst, c.seed_prev, 32, hipMemcpyDeviceToDevice, st));
        // (the owner knows events by the FIELD that holds them: both slots hold one before the handles change places, so that the
        //  release finds a live handle in every field it recorded)
        for (hipEvent_t &e : w->ev_seed[slot]) if (int rce = lazy_event(w->mem, e, hipEventDefault)) return rce;
        for (int q = 0; q < 2; q++) std::swap(w->ev_seed[slot][q], w->ev_seed[from][q]);
    }
    *seed_dev = dst;
    return H2V_OK;
}
// One pass of a mixed call on `st`: the gather kernels behind the tables, then the schedule of the workspace's kind.
static int mixed_enqueue(const MixedCall &c, MixedTables &t, h2v_workspace *w, hipStream_t st) {
    MixedWs *m = w->mixed;
    const h2v_batch &in = c.in;
    if (!c.host_off) hipLaunchKernelGGL(k_mixed_offsets, dim3(1), dim3(256), 0, st, in.proof_off, t.tab, t.d_off);
    hipLaunchKernelGGL(k_mixed_gather, dim3((c.pt.n + 3) / 4), dim3(256), 0, st, t.tab, in.proofs, in.proof_off, in.instances, in.committed, m->proofs.p, (const uint64_t *)t.d_off, m->inst.p, m->ci.p);
    if (hipGetLastError() != hipSuccess) return fail(H2V_E_DEVICE, "launch of the gather kernels failed");
    MixedUnits mu;
    mixed_units(c, t, m, mu);
    if (c.keyed) {      // (the records of the pass: one per phase-1 unit, then the tail's - on either kind of workspace)
        if (int rc = mixed_seed(c, t, w, st, mu.phase1.size() + 1, &mu.fc.seed_dev)) return rc;
        mu.tail.seed_dev = mu.fc.seed_dev; mu.tail.seed_xor7 = 0;
    }
    return w->n_lanes ? mixed_run_laned(c, mu, w, st) : mixed_run_ordinary(mu, w, st);
}
static int run_mixed(const MixedCall &c, h2v_workspace *w, hipStream_t st) {
    int rc;
    if (w->n_lanes && (rc = co_flush(w))) return rc;       // (calls start in submission order: the open groups of coalesced calls first)
    if ((rc = mixed_ensure(w, c.pt))) return rc;
    if (c.rlc && (rc = rlc_stats_ensure(w))) return rc;
    if (c.fold && (rc = mixed_fold_ensure(w, c.lay))) return rc;
    if (c.across && (rc = across_ensure(w, c.cls, !c.fold))) return rc;
    MixedTables t;
    if ((rc = mixed_tables(c, w, st, t))) return rc;
    // from here on the block is in use: THE return records its end on `st` (after an error: drained first)
    rc = mixed_enqueue(c, t, w, st);
    if (rc == H2V_OK && c.keyed) rec_last(w).derived = true;      // (the tail's record: the call's last, whose slot holds the seed)
    if (rc) rc = drain_after_error(w, rc);
    if (hipEventRecord(t.sl->done, st) != hipSuccess && !rc) rc = fail(H2V_E_DEVICE, "event record failed");
    return rc;
}
// argument checks shared by the forms; on success (and b->n != 0) c holds the plans, the flags and the partition
static int mixed_args(const h2v_plan *const *plans, uint32_t n_plans, const h2v_mixed_batch *b, const uint8_t *accept, uint32_t flags, MixedCall *c) {
    h2vmixed::Partition *pt = &c->pt;
    c->plans = plans; c->plan_of = b ? b->plan_of : nullptr;
    c->rlc = (flags & H2V_MIXED_RLC) != 0; c->fold = (flags & H2V_MIXED_FOLD_MSM) != 0; c->grouped = (flags & H2V_MIXED_GROUPED) != 0;
    c->across = (flags & H2V_MIXED_ACROSS_SRS) != 0;
    if (!plans || !b || !accept) return fail(H2V_E_ARG, "null argument");
    const uint32_t max_plans = (flags & H2V_MIXED_GROUPED) ? H2V_MIXED_GROUPED_MAX_PLANS : H2V_MIXED_MAX_PLANS;
    if (n_plans > max_plans)
        return fail(H2V_E_LIMIT, "at most " + std::to_string(max_plans) + " plans in one mixed call" + ((flags & H2V_MIXED_GROUPED) ? " with H2V_MIXED_GROUPED (" : " (") +
                                     std::to_string(n_plans) + " listed)");
    if (flags & ~(H2V_MIXED_RLC | H2V_MIXED_FOLD_MSM | H2V_MIXED_GROUPED | H2V_MIXED_ACROSS_SRS)) return fail(H2V_E_ARG, "unknown flag");
    if ((flags & H2V_MIXED_FOLD_MSM) && !(flags & H2V_MIXED_RLC)) return fail(H2V_E_ARG, "H2V_MIXED_FOLD_MSM is valid only together with H2V_MIXED_RLC");
    if ((flags & H2V_MIXED_GROUPED) && (flags & (H2V_MIXED_RLC | H2V_MIXED_FOLD_MSM)) != (H2V_MIXED_RLC | H2V_MIXED_FOLD_MSM))
        return fail(H2V_E_ARG, "H2V_MIXED_GROUPED is valid only together with H2V_MIXED_RLC | H2V_MIXED_FOLD_MSM");
    if ((flags & H2V_MIXED_ACROSS_SRS) && !(flags & H2V_MIXED_RLC)) return fail(H2V_E_ARG, "H2V_MIXED_ACROSS_SRS is valid only together with H2V_MIXED_RLC");
    if (b->n == 0) return H2V_OK;
    if (n_plans == 0) return fail(H2V_E_ARG, "no plan listed");
    if ((flags & H2V_MIXED_RLC) && b->n > (1ull << 22)) return fail(H2V_E_LIMIT, "RLC batches are limited to 2^22 proofs");
    if (!b->plan_of || !b->proofs || !b->proof_off) return fail(H2V_E_ARG, "null plan_of / proofs / offsets");
    std::vector<h2vmixed::PlanShape> shapes(n_plans);
    for (uint32_t k = 0; k < n_plans; k++) {
        if (!plans[k]) return fail(H2V_E_ARG, "null plan (plans[" + std::to_string(k) + "])");
        ALIVE(plans[k]);
        if (plans[k]->device != plans[0]->device) return fail(H2V_E_ARG, "plans[" + std::to_string(k) + "] lives on another device than plans[0]: one device per call");
        if (!c->across && memcmp(plans[k]->sg2_digest, plans[0]->sg2_digest, sizeof plans[0]->sg2_digest))
            return fail(H2V_E_ARG, "plans[0] and plans[" + std::to_string(k) + "] are on different SRS (their s_g2 differ): one SRS per mixed call");
        shapes[k] = {plans[k]->d.proof_len, plans[k]->d.n_pi, plans[k]->d.n_ci};
    }
    std::string err;
    if (!h2vmixed::partition(shapes.data(), n_plans, b->plan_of, b->n, *pt, &err)) return fail(H2V_E_ARG, err);
    if (c->across) {         // the SRS classes of the call (h2v_mixed_srs.hpp): at most H2V_MULTI_SRS_MAX of them may have proofs
        static_assert(sizeof(h2vsrs::Digest) == sizeof plans[0]->sg2_digest, "a class is one s_g2 digest");
        std::vector<h2vsrs::Digest> dg(n_plans);
        for (uint32_t k = 0; k < n_plans; k++) memcpy(&dg[k], plans[k]->sg2_digest, sizeof(h2vsrs::Digest));
        bool limit = false;
        if (!h2vsrs::classes(dg.data(), *pt, b->plan_of, H2V_MULTI_SRS_MAX, c->cls, &limit, &err)) return fail(limit ? H2V_E_LIMIT : H2V_E_ARG, err);
    }
    if (pt->inst_total && !b->instances) return fail(H2V_E_ARG, "a plan of the call has public inputs but instances == NULL");
    if (pt->ci_total && !b->committed) return fail(H2V_E_ARG, "a plan of the call has a committed instance but committed == NULL");
    return H2V_OK;
}
static int mixed_no_host_batch(const h2v_workspace *ws) {
    if (ws->pending) return fail(H2V_E_ARG, "the workspace has a host batch in flight: call h2v_verify_batch_wait first");
    return H2V_OK;
}
static int mixed_ws_check(const h2v_plan *const *plans, uint32_t n_plans, uint64_t n, const h2v_workspace *ws) {
    for (uint32_t k = 0; k < n_plans; k++)
        if (int rc = ws_fits(ws, plans[k], n, false)) return fail(rc, "plans[" + std::to_string(k) + "]: " + g_err);
    return mixed_no_host_batch(ws);
}
// H2V_MIXED_FOLD_MSM: the layout of the call's term pool on workspace w (h2v_mixed_fold.hpp) - which plans have the batch form
// (rlc_supported), where their terms and block sums go, N_R - decided on the host before anything is enqueued: H2V_E_LIMIT above
// 2^22 terms.
static int mixed_fold_layout(const h2v_plan *const *plans, const h2vmixed::Partition &pt, const h2v_workspace *w, h2vmixed::FoldLayout *lay) {
    std::vector<h2vmixed::FoldShape> shapes(pt.n_plans);
    for (uint32_t k = 0; k < pt.n_plans; k++) shapes[k] = {plans[k]->n_var, plans[k]->n_fix, rlc_supported(plans[k])};
    std::string err;
    if (!h2vmixed::fold_layout(shapes.data(), pt.count.data(), pt.n_plans, w->n_lanes ? w->chunk : 0u, *lay, &err)) return fail(H2V_E_LIMIT, err);
    return H2V_OK;
}
// H2V_MIXED_GROUPED, on the host before anything is enqueued: which plans are groupable (foldable, register file in LDS), the
// grouped positions, and the fold layout's block sums re-cut along the ranges of those positions.  The records of a call: one for
// the grouped part, one per other plan with proofs, the tail's - and the ring holds RING of them: more than
// H2V_MIXED_GROUPED_MAX_OTHER other plans with proofs is H2V_E_LIMIT.
static_assert(H2V_MIXED_GROUPED_MAX_OTHER + 2 <= h2v_workspace::RING, "a grouped call's records fit the ring");
static int mixed_group_layout(const h2v_plan *const *plans, const h2vmixed::Partition &pt, h2vmixed::FoldLayout *lay, MixedGroupPlan *gp) {
    gp->shapes.resize(pt.n_plans);
    for (uint32_t k = 0; k < pt.n_plans; k++) gp->shapes[k] = {plans[k]->d, plans[k]->n_var, plans[k]->n_fix, vm_lds_slots(plans[k]->d), rlc_supported(plans[k])};
    h2vmixed::group_space(gp->shapes.data(), pt.count.data(), pt.n_plans, lay->chunk, gp->sp);
    if (gp->sp.n_other > H2V_MIXED_GROUPED_MAX_OTHER)
        return fail(H2V_E_LIMIT, "at most " + std::to_string(H2V_MIXED_GROUPED_MAX_OTHER) + " plans that cannot be grouped (recursive, or with a global register file) may have proofs in one call, this one has " +
                                     std::to_string(gp->sp.n_other));
    h2vmixed::group_fold_blocks(gp->sp, gp->shapes.data(), pt.count.data(), *lay);
    return H2V_OK;
}
// One mixed call on `st`.  c.fold (H2V_MIXED_FOLD_MSM): the fold form first - one bucket MSM and one pairing for the call - and then
// the HOST decides: the record's verdict word comes down and `st` is synchronised (the one synchronisation of the form; phase-1
// results no longer exist by then, the lanes have recycled them).  Passed: accept[] / status[] are final.  Failed: the
// H2V_MIXED_RLC path runs on the same inputs with the same seed - its pair check, group stage and per-pair kernels localise the
// rejects -, *fold_failed is set and the call's last record is that second pass's.
static int run_mixed_call(const MixedCall &c, h2v_workspace *w, hipStream_t st, bool *fold_failed) {
    int rc = run_mixed(c, w, st);
    if (rc || !c.fold) return rc;
    uint32_t failed = 0;
    if (verdict_down(w, &failed, st) || hipStreamSynchronize(st) != hipSuccess)
        return drain_after_error(w, fail(H2V_E_DEVICE, "mixed-call kernels failed (fold form)"));
    if (!failed) return H2V_OK;
    if (fold_failed) *fold_failed = true;
    MixedCall second = c;
    second.fold = second.grouped = false;
    const uint64_t first_tail = rec_last(w).call;
    if (c.keyed) second.seed_prev = w->seed_ring + (size_t)(first_tail % h2v_workspace::RING) * 8;      // (derived once per call)
    rc = run_mixed(second, w, st);
    if (c.keyed && rc == H2V_OK)
        if (CallRec *r = rec_at(w, first_tail)) r->derived = false;      // (the seed and its events are the second tail's now)
    return rc;
}
// the layouts of a call on workspace ws, on the host before anything is enqueued: the fold form's, then the grouped form's
static int mixed_layouts(MixedCall &c, const h2v_workspace *ws) {
    if (c.fold)
        if (int rc = mixed_fold_layout(c.plans, c.pt, ws, &c.lay)) return rc;
    return c.grouped ? mixed_group_layout(c.plans, c.pt, &c.lay, &c.grp) : (int)H2V_OK;
}
// The last step of filling a MixedCall: its I/O.  THE place where the combinations of its parts are checked: the grouped form
// needs the fold layout (cut at the same chunk size), an aggregate call needs it, and the fold form needs the coefficients.
static int mixed_call_io(MixedCall &c, const h2v_batch &in, const uint64_t *host_off, uint8_t *accept, uint32_t *status, uint32_t *agg_parts) {
    c.in = in; c.host_off = host_off; c.accept = accept; c.status = status; c.agg_parts = agg_parts;
    if (c.grouped && (!c.fold || c.grp.sp.chunk != c.lay.chunk)) return fail(H2V_E_DEVICE, "internal: grouped call without its fold layout");
    if (c.agg_parts && !c.fold) return fail(H2V_E_DEVICE, "internal: aggregate call without its fold layout");
    if (c.fold && !c.rlc) return fail(H2V_E_DEVICE, "internal: fold form without its coefficients");
    return H2V_OK;
}
// what H2V_MIXED_* flags an aggregate-mixed call is: the grouped fold form, H2V_RLC_GROUPED asking for the grouping
static uint32_t agg_mixed_flags(const h2v_rlc_opts *opts) {
    return H2V_MIXED_RLC | H2V_MIXED_FOLD_MSM | (opts && (opts->flags & H2V_RLC_GROUPED) ? H2V_MIXED_GROUPED : 0u);
}
extern "C" int h2v_verify_mixed_device(const h2v_plan *const *plans, uint32_t n_plans, const h2v_mixed_batch *b, uint8_t *accept, uint32_t *status,
                                       h2v_workspace *ws, void *stream, uint32_t flags, const h2v_rlc_opts *opts) {
    MixedCall c;
    if (int rcs = seed_flags_mixed(opts, (flags & H2V_MIXED_RLC) != 0, &c.keyed)) return rcs;
    int rc = mixed_args(plans, n_plans, b, accept, flags, &c);
    if (rc || b->n == 0) return rc;
    if (!ws) return fail(H2V_E_ARG, "the device form needs a workspace (h2v_workspace_create_multi over the listed plans)");
    ALIVE(ws);
    HIPCHK(hipSetDevice(plans[0]->device));
    if ((rc = mixed_ws_check(plans, n_plans, b->n, ws))) return rc;
    if ((rc = null_stream_check(ws, stream))) return rc;
    if (c.rlc && !c.keyed && (rc = rlc_seed(opts, c.seed))) return rc;      // (the device forms: the seed before the layouts)
    if ((rc = mixed_layouts(c, ws))) return rc;
    if ((rc = mixed_call_io(c, {b->n, b->proofs, b->proof_off, b->instances, b->committed}, nullptr, accept, status, nullptr))) return rc;
    return run_mixed_call(c, ws, (hipStream_t)stream, nullptr);
}
// Host-buffer form: offsets | instances | committed | proofs go up in one pinned block on the workspace's own stream, the call
// runs there behind it, and accept[] / status[] / the batch verdict come back before the function returns.
// agg_pair (h2v_aggregate_mixed): the fold form without its verdict - `accept` is the caller's included[], the call's pair comes
// back in agg_pair and nothing is checked, downloaded in between or run a second time.
static int agg_info_fill(h2v_aggregate_info *info, const uint32_t seed[8], uint32_t chunk, uint32_t nch, uint64_t terms, bool derived = false);
struct AggSlot { uint32_t *parts; uint32_t slot; };
static int agg_export(h2v_workspace *ws, const AggSlot &a, uint32_t n_parts, uint8_t *d_pair, hipStream_t st);
static int agg_ensure(h2v_workspace *ws, uint32_t n_parts, hipStream_t st, AggSlot *out);
static int mixed_host(const h2v_plan *const *plans, uint32_t n_plans, const h2v_mixed_batch *b, uint8_t *accept, uint32_t *status,
                      h2v_workspace *ws, uint32_t flags, const h2v_rlc_opts *opts, int *fell_back, uint8_t *agg_pair, h2v_aggregate_info *info) {
    if (fell_back) *fell_back = 0;
    MixedCall c;
    if (int rcs = seed_flags_mixed(opts, (flags & H2V_MIXED_RLC) != 0, &c.keyed)) return rcs;
    const h2vmixed::Partition &pt = c.pt;
    int rc = mixed_args(plans, n_plans, b, accept, flags, &c);
    if (rc || b->n == 0) return rc;
    ALIVE(ws);
    HIPCHK(hipSetDevice(plans[0]->device));
    const uint64_t n = b->n;
    h2v_workspace *tmp = nullptr;
    if (!ws) {    // a temporary workspace over the listed plans: lanes of at most the call's size, created as they are used
        if ((rc = h2v_workspace_create_multi(plans, n_plans, n, 0, n < 4096 ? (uint32_t)n : 4096u, &tmp))) return rc;
        ws = tmp;
    }
    bool fold_failed = false;
    h2v_batch in{};
    hostcall::ResultBlock R;
    rc = mixed_ws_check(plans, n_plans, n, ws);
    if (rc == H2V_OK) rc = mixed_layouts(c, ws);                 // (the host form: the layouts before the seed)
    if (rc == H2V_OK && c.rlc && !c.keyed) rc = rlc_seed(opts, c.seed);
    if (rc == H2V_OK) rc = mixed_ensure(ws, pt);
    if (rc == H2V_OK) rc = result_ensure(ws, hostcall::Call::MIXED, n, &R, ws->mixed);
    if (rc == H2V_OK) {
        const h2v_batch hb = {n, b->proofs, b->proof_off, b->instances, b->committed};
        rc = stage_batch(&hb, pt.inst_total, (size_t)pt.ci_total * 48, ws, ws->mixed->in, &in, ws->mixed);
    }
    if (rc == H2V_OK) {
        std::vector<uint64_t> goff(n + 1);
        h2vmixed::group_offsets(pt, (const uint64_t *)ws->mixed->in.h_block.p, goff.data());     // (the packed offsets: rebased)
        uint8_t *const d = ws->res.p, *d_accept = d + R.accept.off;
        uint32_t *d_status = (uint32_t *)(d + R.status.off);
        if (agg_pair) {      // (run_mixed, not run_mixed_call: no verdict comes down and nothing runs a second time)
            AggSlot as{};
            if ((rc = agg_ensure(ws, 1, ws->hs, &as)) == H2V_OK) rc = mixed_call_io(c, in, goff.data(), d_accept, d_status, as.parts);
            if (rc == H2V_OK) rc = run_mixed(c, ws, ws->hs);
            if (rc == H2V_OK) rc = agg_export(ws, as, 1, d + R.pairs.off, ws->hs);
            if (rc == H2V_OK) rc = agg_info_fill(info, c.seed, 0, 1, c.lay.n_r, c.keyed);
        } else if ((rc = mixed_call_io(c, in, goff.data(), d_accept, d_status, nullptr)) == H2V_OK) rc = run_mixed_call(c, ws, ws->hs, &fold_failed);
        rc = host_call_tail(ws, rc, {{agg_pair, R.pairs, "the pair"}, {accept, R.accept, "accept[]"}, {status, R.status, "the status words"}},
                            c.rlc && !agg_pair, fell_back, "mixed-call", fold_failed);
        if (rc == H2V_OK && agg_pair && info && c.keyed) rc = h2v_workspace_seed_used(ws, 0, info->seed_used);      // (the stream is synchronised: the derived seed is there)
    }
    if (tmp) h2v_workspace_free(tmp);
    return rc;
}
extern "C" int h2v_verify_mixed(const h2v_plan *const *plans, uint32_t n_plans, const h2v_mixed_batch *b, uint8_t *accept, uint32_t *status,
                                h2v_workspace *ws, uint32_t flags, const h2v_rlc_opts *opts, int *fell_back) {
    return mixed_host(plans, n_plans, b, accept, status, ws, flags, opts, fell_back, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------- aggregate calls
// h2v_aggregate_batch(_device) / h2v_aggregate_mixed(_device): the batch-accept forms up to and including their bucket MSMs, and
// then the batch's pair  compress(L) || compress(R),  L = sum r_i L_i, R = sum r_i R_i,  instead of a pairing on it - "prepare the
// batch's pair" beside h2v_prepare_batch's "prepare every proof's pair"; h2v_check_pairs(_rlc) checks pairs from anywhere.  The
// pipelines are run_rlc, run_pipeline + fold_pairs_tail (recursive plans) and run_mixed with the fold layout, unchanged up to
// pip_launch; agg_chunk ends every unit, and ONE k_aggregate_export per call (h2v_aggregate_dev.hpp) adds the units' sums and
// writes the pair, on the caller's stream behind the call's lanes.  Never routed, never coalesced; no estimate moves.
// THE INVARIANT of the parts buffer: slot q is the FIXED range [q * AGG_SLOT_PARTS, (q + 1) * AGG_SLOT_PARTS) of it, whatever the
// calls' sizes, and ev_agg[q] - while agg_used[q] - is recorded behind the last export that read anything in that range.  A call of
// at most AGG_SLOT_PARTS parts takes ONE slot (round robin) and waits for that slot's event; a larger call takes the WHOLE buffer
// from its start (every slot and what lies behind them), waits for every used event and records every event behind its export.  So
// whoever writes a range has waited, on its own stream, for every export that read it - on whatever streams the calls arrive and in
// whatever order their sizes change.  Growing the buffer (a larger call only) waits on the host for those same events: every export
// so far, and with them the copies of their chunks, are done; no other stream of the process is touched.
static int agg_ensure(h2v_workspace *ws, uint32_t n_parts, hipStream_t st, AggSlot *out) {
    constexpr uint32_t S = h2v_workspace::AGG_SLOTS, P = h2v_workspace::AGG_SLOT_PARTS;
    const uint32_t per = n_parts ? n_parts : 1u, need = per <= P ? S * P : per;
    for (hipEvent_t &e : ws->ev_agg) if (int rce = lazy_event(ws->mem, e, hipEventDisableTiming)) return rce;
    if (int rc = ws->agg_parts.ensure(ws->mem, (size_t)need * AGG_PART_DW * 4, "the aggregate parts", [&]() -> int {
            for (uint32_t q = 0; q < S; q++)
                if (ws->agg_used[q]) { HIPCHK(hipEventSynchronize(ws->ev_agg[q])); ws->agg_used[q] = false; }
            return H2V_OK;
        })) return rc;
    uint32_t *const parts = (uint32_t *)ws->agg_parts.p;
    if (per <= P) {
        out->slot = (uint32_t)(ws->agg_calls++ % S);
        out->parts = parts + (size_t)out->slot * P * AGG_PART_DW;
        if (ws->agg_used[out->slot]) HIPCHK(hipStreamWaitEvent(st, ws->ev_agg[out->slot], 0));
    } else {
        out->slot = S;      // the whole buffer
        out->parts = parts;
        for (uint32_t q = 0; q < S; q++)
            if (ws->agg_used[q]) HIPCHK(hipStreamWaitEvent(st, ws->ev_agg[q], 0));
    }
    return H2V_OK;
}
static int agg_export(h2v_workspace *ws, const AggSlot &a, uint32_t n_parts, uint8_t *d_pair, hipStream_t st) {
    constexpr uint32_t S = h2v_workspace::AGG_SLOTS;
    hipLaunchKernelGGL(k_aggregate_export, dim3(1), dim3(256), 0, st, (const uint32_t *)a.parts, n_parts, (uint32_t *)d_pair);
    HIPCHK(hipGetLastError());
    for (uint32_t q = a.slot < S ? a.slot : 0; q < (a.slot < S ? a.slot + 1 : S); q++) {
        HIPCHK(hipEventRecord(ws->ev_agg[q], st));
        ws->agg_used[q] = true;
    }
    return H2V_OK;
}
static int agg_info_fill(h2v_aggregate_info *info, const uint32_t seed[8], uint32_t chunk, uint32_t nch, uint64_t terms, bool derived) {
    if (!info) return H2V_OK;
    memset(info, 0, sizeof *info);
    if (!derived) memcpy(info->seed_used, seed, 32);      // (a derived seed is not known yet: zeros; h2v_workspace_seed_used has it)
    info->reserved = derived ? 1u : 0u;                                                                        // (the seed source)
    info->chunk = chunk; info->n_chunks = nch; info->msm_terms = (uint32_t)terms;
    return H2V_OK;
}
static void agg_pair_inf(uint8_t pair[96]) { memset(pair, 0, 96); pair[0] = 0xc0; pair[48] = 0xc0; }
// (mixed: h2v_aggregate_mixed(_device), the one call that knows H2V_RLC_GROUPED)
static int agg_flags(const h2v_rlc_opts *o, bool mixed = false, bool *keyed = nullptr) {
    if (mixed) {
        if (int rc = seed_flags_mixed(o, true, keyed)) return rc;
    } else if (int rc = seed_keyed_refused(o)) return rc;
    if (o && (o->flags & ~(H2V_RLC_SEED_GIVEN | H2V_RLC_ONE_STREAM | H2V_RLC_FOLD_PAIRS | (mixed ? H2V_RLC_GROUPED | H2V_RLC_SEED_KEYED : H2V_RLC_SEED_TRANSCRIPT))))
        return fail(H2V_E_ARG, "unknown flag in h2v_rlc_opts.flags");
    bool derive;
    return mixed ? (int)H2V_OK : seed_flags(o, &derive);
}
// the argument rules of the single-key forms that need no device
static int agg_batch_args(const h2v_plan *p, const h2v_batch *b, const uint8_t *pair, const uint8_t *included, const h2v_rlc_opts *opts) {
    if (int rck = seed_keyed_refused(opts)) return rck;      // (named before anything else: the mixed calls' flag in a single-key call)
    if (!p) return fail(H2V_E_ARG, "null argument: plan");
    if (!b) return fail(H2V_E_ARG, "null argument: batch");
    if (!pair) return fail(H2V_E_ARG, "null argument: pair");
    if (b->n && !included) return fail(H2V_E_ARG, "null argument: included");
    if (int rc = agg_flags(opts)) return rc;
    if (b->n > (1ull << 22)) return fail(H2V_E_LIMIT, "RLC batches are limited to 2^22 proofs");
    if (b->n)
        if (int rc = batch_args(p, b)) return rc;
    if (b->n && !rlc_supported(p) && !p->d.ivc) return fail(H2V_E_ARG, "this plan has no batch form (its VK-base terms are not the tail of its term list)");
    return H2V_OK;
}
// One single-key aggregate call on `st`: device-resident batch `in` of n > 0 proofs, d_pair / d_included / d_status device memory.
// A laned workspace: the chunks through the lanes, `st` joined inside the call (the per-chunk sums must meet), then the export.
static int agg_run(const h2v_plan *p, const h2v_batch *in, uint8_t *d_pair, uint8_t *d_included, uint32_t *d_status, h2v_workspace *ws, hipStream_t st,
                   const h2v_rlc_opts *opts, h2v_aggregate_info *info) {
    const uint32_t n = (uint32_t)in->n, nch = ws->n_lanes ? n_chunks(n, ws->chunk) : 1u;
    Unit u = unit_of_batch(rlc_supported(p) ? UnitKind::RLC : UnitKind::FOLD_RLC, p, in, d_included, d_status);
    u.one_stream_opt = opts && (opts->flags & H2V_RLC_ONE_STREAM);
    int rc = seed_flags(opts, &u.derive);
    if (rc == H2V_OK && !u.derive) rc = rlc_seed(opts, u.seed);
    if (rc) return rc;
    agg_info_fill(info, u.seed, ws->n_lanes ? ws->chunk : 0u, nch, u.kind == UnitKind::RLC ? (uint64_t)n * p->n_var + (uint64_t)nch * p->n_fix : (uint64_t)n, u.derive);
    if ((rc = rlc_stats_ensure(ws))) return rc;      // (the records' verdict words)
    AggSlot as{};
    if ((rc = agg_ensure(ws, nch, st, &as))) return rc;
    u.agg_parts = as.parts;
    if ((rc = run_call(u, ws, st, Join::NOW))) return rc;
    return agg_export(ws, as, nch, d_pair, st);
}
extern "C" int h2v_aggregate_batch_device(const h2v_plan *p, const h2v_batch *b, uint8_t *pair, uint8_t *included, uint32_t *status, h2v_workspace *ws,
                                          void *stream, const h2v_rlc_opts *opts, h2v_aggregate_info *info) {
    int rc = agg_batch_args(p, b, pair, included, opts);
    if (rc) return rc;
    if ((uintptr_t)pair & 3) return fail(H2V_E_ARG, "pair must be 4-byte aligned");
    if (!ws) return fail(H2V_E_ARG, "the device form needs a workspace");
    ALIVE(p); ALIVE(ws);
    HIPCHK(hipSetDevice(p->device));
    if (b->n && (rc = ws_fits(ws, p, b->n, false))) return rc;
    if (ws->pending) return fail(H2V_E_ARG, "the workspace has a host batch in flight: call h2v_verify_batch_wait first");
    if ((rc = null_stream_check(ws, stream))) return rc;
    if (b->n == 0) {       // nothing is included: (inf, inf), which h2v_check_pairs accepts
        uint32_t seed[8];
        if ((rc = rlc_seed(opts, seed))) return rc;
        agg_info_fill(info, seed, ws->n_lanes ? ws->chunk : 0u, 1u, 0);
        AggSlot as{};
        if ((rc = agg_ensure(ws, 1, (hipStream_t)stream, &as))) return rc;
        return agg_export(ws, as, 0, pair, (hipStream_t)stream);
    }
    return agg_run(p, b, pair, included, status, ws, (hipStream_t)stream, opts, info);
}
// Host-buffer form: staged as h2v_prepare_batch stages its batch; pair, included[] and status[] come back before the call returns.
extern "C" int h2v_aggregate_batch(const h2v_plan *p, const h2v_batch *b, uint8_t pair[96], uint8_t *included, uint32_t *status, h2v_workspace *ws,
                                   const h2v_rlc_opts *opts, h2v_aggregate_info *info) {
    int rc = agg_batch_args(p, b, pair, included, opts);
    if (rc) return rc;
    const uint64_t n = b->n;
    if (n == 0) {
        uint32_t seed[8];
        if ((rc = rlc_seed(opts, seed))) return rc;
        agg_info_fill(info, seed, ws && ws->n_lanes ? ws->chunk : 0u, 1u, 0);
        agg_pair_inf(pair);
        return H2V_OK;
    }
    TmpWs tmp;
    if ((rc = pairs_common(p, n, ws, nullptr, false, tmp))) return rc;
    h2v_batch in{};
    hostcall::ResultBlock R;
    rc = result_ensure(ws, hostcall::Call::AGGREGATE, n, &R);
    if (rc == H2V_OK) rc = stage_batch(p, b, ws, own_slot(ws), &in);
    if (rc) return rc;
    uint8_t *const d = ws->res.p;
    rc = agg_run(p, &in, d + R.pairs.off, d + R.accept.off, (uint32_t *)(d + R.status.off), ws, ws->hs, opts, info);
    rc = host_call_tail(ws, rc, {{pair, R.pairs, "the pair"}, {included, R.accept, "included[]"}, {status, R.status, "the status words"}}, false, nullptr, "aggregate");
    if (rc == H2V_OK && info && H2V_AGGREGATE_SEED_SOURCE(info) == 1) rc = h2v_workspace_seed_used(ws, 0, info->seed_used);      // (the stream is synchronised: the derived seed is there)
    return rc;
}
extern "C" int h2v_aggregate_mixed_device(const h2v_plan *const *plans, uint32_t n_plans, const h2v_mixed_batch *b, uint8_t *pair, uint8_t *included,
                                          uint32_t *status, h2v_workspace *ws, void *stream, const h2v_rlc_opts *opts, h2v_aggregate_info *info) {
    if (!pair) return fail(H2V_E_ARG, "null argument: pair");
    if (b && b->n == 0 && !included) included = pair;      // (nothing to write; mixed_args wants a pointer)
    MixedCall c;
    if (int rca = agg_flags(opts, true, &c.keyed)) return rca;
    int rc = mixed_args(plans, n_plans, b, included, agg_mixed_flags(opts), &c);
    if (rc) return rc;
    if ((uintptr_t)pair & 3) return fail(H2V_E_ARG, "pair must be 4-byte aligned");
    if (!ws) return fail(H2V_E_ARG, "the device form needs a workspace (h2v_workspace_create_multi over the listed plans)");
    ALIVE(ws);
    // ws->device, where the other forms say plans[0]->device: a call of NO proofs runs too (it exports the pair (inf, inf)), and it
    // may list no plan at all.  With proofs the two are equal: mixed_ws_check -> ws_fits holds every plan to the workspace's device.
    HIPCHK(hipSetDevice(ws->device));
    if ((rc = b->n ? mixed_ws_check(plans, n_plans, b->n, ws) : mixed_no_host_batch(ws))) return rc;   // (no proofs: no plan to fit)
    if ((rc = null_stream_check(ws, stream))) return rc;
    if (!c.keyed && (rc = rlc_seed(opts, c.seed))) return rc;
    AggSlot as{};
    if (b->n == 0) {      // (keyed: nothing is derived from no proofs - seed_used stays zero)
        agg_info_fill(info, c.seed, 0, 1, 0);
        if ((rc = agg_ensure(ws, 1, (hipStream_t)stream, &as))) return rc;
        return agg_export(ws, as, 0, pair, (hipStream_t)stream);
    }
    if ((rc = mixed_layouts(c, ws))) return rc;
    agg_info_fill(info, c.seed, 0, 1, c.lay.n_r, c.keyed);
    if ((rc = agg_ensure(ws, 1, (hipStream_t)stream, &as))) return rc;
    if ((rc = mixed_call_io(c, {b->n, b->proofs, b->proof_off, b->instances, b->committed}, nullptr, included, status, as.parts))) return rc;
    // (run_mixed, not run_mixed_call: no verdict comes down, the stream is not synchronised and nothing runs a second time)
    if ((rc = run_mixed(c, ws, (hipStream_t)stream))) return rc;
    return agg_export(ws, as, 1, pair, (hipStream_t)stream);
}
extern "C" int h2v_aggregate_mixed(const h2v_plan *const *plans, uint32_t n_plans, const h2v_mixed_batch *b, uint8_t pair[96], uint8_t *included,
                                   uint32_t *status, h2v_workspace *ws, const h2v_rlc_opts *opts, h2v_aggregate_info *info) {
    if (!pair) return fail(H2V_E_ARG, "null argument: pair");
    if (int rca = agg_flags(opts, true)) return rca;
    const uint32_t mflags = agg_mixed_flags(opts);
    if (b && b->n == 0) {      // (inf, inf) without a device; the argument rules still hold
        MixedCall none;
        if (int rc = mixed_args(plans, n_plans, b, pair, mflags, &none)) return rc;
        uint32_t seed[8] = {};
        if (!(opts && (opts->flags & H2V_RLC_SEED_KEYED)))      // (keyed: nothing is derived from no proofs - seed_used stays zero)
            if (int rc = rlc_seed(opts, seed)) return rc;
        agg_info_fill(info, seed, 0, 1, 0);
        agg_pair_inf(pair);
        return H2V_OK;
    }
    return mixed_host(plans, n_plans, b, included, status, ws, mflags, opts, nullptr, pair, info);
}

// After the stream of an RLC call has been synchronised: did the batch check pass (1) or did the per-proof kernels run (0)?
// kernel times of a past call (calls_back = 0: the most recent).
static int rec_rlc_timings(const CallRec &r, h2v_rlc_timings *tm);
extern "C" int h2v_workspace_rlc_result(h2v_workspace *w, uint32_t calls_back, uint32_t *batch_accepted, h2v_rlc_timings *tm) {
    if (!w) return fail(H2V_E_ARG, "null argument");
    ALIVE(w);
    const CallRec *r;
    if (int rc = rec_lookup(w, calls_back, &r)) return rc;
    if (r->kind != h2v_workspace::RLC) return fail(H2V_E_ARG, "that call did not run in RLC mode");
    if (r->routed) {       // routed to the per-proof kernels: no batch check ran (h2v_workspace_timings has its times)
        if (batch_accepted) *batch_accepted = 0;
        if (tm) memset(tm, 0, sizeof *tm);
        return H2V_OK;
    }
    HIPCHK(hipSetDevice(w->device));
    if (batch_accepted && r->agg) *batch_accepted = H2V_BATCH_NOT_CHECKED;   // (an aggregate call: the pair was exported, no pairing ran)
    else if (batch_accepted) {   // (laned: the AND of the chunks' batch verdicts)
        uint32_t failed = 0;
        HIPCHK(hipMemcpy(&failed, rec_word(w, *r), 4, hipMemcpyDeviceToHost));
        *batch_accepted = failed == 0 ? 1u : 0u;
    }
    if (!tm) return H2V_OK;
    if (!w->n_lanes) return rec_rlc_timings(*r, tm);
    // laned: times summed over the chunks, total = first start .. last verdict
    memset(tm, 0, sizeof *tm);
    hipEvent_t first = nullptr;
    int rc = each_chunk(w, *r, [&](const CallRec &lr) -> int {
        h2v_rlc_timings t1;
        if (int rc1 = rec_rlc_timings(lr, &t1)) return rc1;
        tm->transcript_combiner_ms += t1.transcript_combiner_ms; tm->g1_decompress_ms += t1.g1_decompress_ms; tm->prepare_ms += t1.prepare_ms;
        tm->bucket_sort_ms += t1.bucket_sort_ms; tm->bucket_accumulate_ms += t1.bucket_accumulate_ms; tm->bucket_reduce_ms += t1.bucket_reduce_ms;
        tm->pairing_ms += t1.pairing_ms;
        tm->msm_terms = t1.msm_terms; tm->window_bits = t1.window_bits; tm->windows = t1.windows; tm->max_chain = t1.max_chain;
        if (!first) first = lr.ev[0];
        float span = 0;
        HIPCHK(hipEventElapsedTime(&span, first, lr.ev[9]));
        if (span > tm->total_ms) tm->total_ms = span;
        return H2V_OK;
    });
    if (rc) return rc;
    if (r->co) {     // a coalesced call: its share of the one batch check that served its group (total_ms: the group's)
        const float f = r->share;
        tm->transcript_combiner_ms *= f; tm->g1_decompress_ms *= f; tm->prepare_ms *= f; tm->bucket_sort_ms *= f;
        tm->bucket_accumulate_ms *= f; tm->bucket_reduce_ms *= f; tm->pairing_ms *= f;
    }
    return H2V_OK;
}
// the times of one batch check of an ordinary workspace (or of a lane): run_rlc's events
static int rec_rlc_timings(const CallRec &r, h2v_rlc_timings *tm) {
    const hipEvent_t *ev = r.ev;
    memset(tm, 0, sizeof *tm);
    HIPCHK(hipEventSynchronize(ev[9]));
    HIPCHK(hipEventElapsedTime(&tm->g1_decompress_ms, ev[0], ev[1]));
    if (!r.no_vm) HIPCHK(hipEventElapsedTime(&tm->transcript_combiner_ms, ev[2], ev[3]));
    HIPCHK(hipEventElapsedTime(&tm->prepare_ms, ev[10], ev[4]));
    HIPCHK(hipEventElapsedTime(&tm->bucket_sort_ms, ev[5], ev[6]));
    HIPCHK(hipEventElapsedTime(&tm->bucket_accumulate_ms, ev[6], ev[7]));
    HIPCHK(hipEventElapsedTime(&tm->bucket_reduce_ms, ev[7], ev[8]));
    if (!r.agg) HIPCHK(hipEventElapsedTime(&tm->pairing_ms, ev[8], ev[9]));   // (an aggregate call: ev[9] closes the copies of its sums)
    float a0, a1;
    HIPCHK(hipEventElapsedTime(&a0, ev[0], ev[9]));
    HIPCHK(hipEventElapsedTime(&a1, ev[2], ev[9]));
    tm->total_ms = a0 > a1 ? a0 : a1;
    tm->msm_terms = r.rlc_terms; tm->window_bits = r.rlc_c; tm->windows = r.rlc_W; tm->max_chain = r.rlc_chain;
    return H2V_OK;
}

// the single-proof trace and the probes of the device code (tests and tools call them)
#include "h2v_probes.hpp"
