// Binary verifier-plan layout shared by the plan compiler (plan.py: Plan.to_bytes) and the HIP backend.
// The plan is this build's "VerifyingKey surface": the reference's InstantiationSpecificData
// (/root/reference/src/plutus_gen/extraction/data/circuit_types/instantiation_data.rs:26-41) plus the
// straight-line verifier program that `extract_circuit` + the emitters would have rendered as source text.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define H2V_PLAN_MAGIC "H2VPLAN1"
#define H2V_PLAN_VERSION 4u
// A plan whose transcript hash is not the Cardano flavour is written as version 5: a library that reads version 4 only
// refuses it instead of replaying its proofs under the wrong hash.  A plan of kind 0 is still written as version 4 with
// the three transcript words zero, byte for byte what earlier builds wrote.  The loader takes both.
#define H2V_PLAN_VERSION_FLAVOURED 5u
// transcript hash H of CircuitTranscript<H> (H2V_HW_TR_KIND; include/h2v.h: H2V_TRANSCRIPT_*)
#define H2V_TR_CARDANO_BLAKE2B_256 0u   // CardanoFriendlyBlake2b: unkeyed blake2b-256, squeeze = h || blake2b-256(h)
#define H2V_TR_BLAKE2B_512 1u           // blake2b_simd::State, 64-byte digest, keyed: squeeze = digest of a copy of the state
#define H2V_TR_KIND_COUNT 2u
#define H2V_TR_KEY_MAX 64u
#define H2V_PLAN_HDR_WORDS 46
#define H2V_MILLER_LINES 68  // 63 doublings + 5 additions for |x| = 0xd201000000010000

// header words (uint32 little-endian) after the 8-byte magic
enum {
    H2V_HW_VERSION = 0, H2V_HW_PROOF_LEN, H2V_HW_N_PI, H2V_HW_N_CI, H2V_HW_N_REGS, H2V_HW_N_INSTR, H2V_HW_N_CONSTS,
    H2V_HW_N_POINTS, H2V_HW_N_VK_BASES, H2V_HW_N_TERMS, H2V_HW_N_TRACE, H2V_HW_PI_POINT, H2V_HW_N_SQUEEZES,
    H2V_HW_STREAM_LEN,
    H2V_HW_OFF_INSTR, H2V_HW_OFF_CONSTS, H2V_HW_OFF_POINTS, H2V_HW_OFF_VK_BASES, H2V_HW_OFF_TERMS, H2V_HW_OFF_LINES_SG2,
    H2V_HW_OFF_LINES_G2, H2V_HW_OFF_TRACE, H2V_HW_TOTAL_LEN, H2V_HW_OFF_LINES28_SG2, H2V_HW_OFF_LINES28_G2,
    // recursion (IVC; plan.py / ivc.py): flag, number of terms of the proof's own MSM, and the public-input positions
    // (x_hi, x_lo, y_hi, y_lo) of the two accumulator points
    H2V_HW_IVC, H2V_HW_N_MAIN_TERMS, H2V_HW_ACC_IDX0 /* .. +7 */,
    // lanes per proof of the transcript + combiner program (the instruction stream is a sequence of bundles of that many
    // records), and an optional second, wider schedule of the same program: lanes (0 = none), registers, records, offset
    H2V_HW_VM_LANES = H2V_HW_ACC_IDX0 + 8, H2V_HW_VM2_LANES, H2V_HW_VM2_N_REGS, H2V_HW_VM2_N_INSTR, H2V_HW_VM2_OFF_INSTR,
    // transcript hash of the key: kind (0 = Cardano), and the blake2b key's byte range in the blob (0, 0 = no key)
    H2V_HW_TR_KIND, H2V_HW_TR_KEY_OFF, H2V_HW_TR_KEY_LEN
};
static_assert(H2V_HW_TR_KIND == 40 && H2V_HW_TR_KEY_LEN < H2V_PLAN_HDR_WORDS, "transcript words are header words 40-42");

// opcodes of the transcript + Fr-combiner program (8-byte records: op, pad, dst, a, b).  The program is a sequence of
// BUNDLES of `vm_lanes` records: record l of a bundle is executed by lane l of the proof's lanes (NOP = idle).  Records of
// one bundle are independent (none reads or writes a register another one writes); the transcript operations (ABSORB_*,
// READ_*, SQUEEZE) and END sit on lane 0 with the rest of their bundle idle.
enum {
    H2V_OP_END = 0, H2V_OP_ABSORB_REG, H2V_OP_ABSORB_CI, H2V_OP_LOAD_INSTANCE, H2V_OP_READ_POINT, H2V_OP_READ_SCALAR,
    H2V_OP_SQUEEZE, H2V_OP_CONST, H2V_OP_ADD, H2V_OP_SUB, H2V_OP_MUL, H2V_OP_NEG, H2V_OP_INV, H2V_OP_OUT_SCALAR,
    H2V_OP_ASSERT_ZERO,  // status |= H2V_ST_RECURSION unless reg a == 0 (verifying-key hash check of the IVC fold)
    H2V_OP_NOP,
    H2V_OP_COUNT
};
// THE opcode table: what each of a record's three fields holds, and where the record may stand.  The loader's validation
// (h2v_planblob.hpp: check_program) and the plan compiler's scheduler and register allocator (h2v_plancc.hpp) read these rows
// and nothing else; plan.py keeps its own lists as the independent model, and tests/test_plan_blob.py compares the two.
// A register in `dst` is WRITTEN by the record, a register in `a` / `b` is READ by it.
enum {
    H2V_ARG_NONE = 0,   // not looked at
    H2V_ARG_REG,        // a register of the program
    H2V_ARG_CONST,      // an index into the constant table
    H2V_ARG_PI,         // an index into the proof's public inputs
    H2V_ARG_TERM,       // an index into the MSM term table
    H2V_ARG_OFF32,      // in `a`: a | b << 16 is the byte offset of a 32-byte scalar in the proof
    H2V_ARG_OFF48       // in `a`: a | b << 16 is the byte offset of a 48-byte point in the proof
};
struct H2vOpInfo {
    uint8_t dst, a, b;    // H2V_ARG_*
    uint8_t serial;       // the bundle rule: stands on lane 0 with the rest of its bundle idle (the transcript operations AND END)
    uint8_t transcript;   // the scheduler: a transcript operation - a bundle of its own, in program order (END is not one: the
                          // scheduler drops it and closes the program itself)
    uint8_t needs_ci;     // only in a plan with a committed instance
};
static constexpr H2vOpInfo H2V_OPS[H2V_OP_COUNT] = {
    /* END           */ {H2V_ARG_NONE, H2V_ARG_NONE, H2V_ARG_NONE, 1, 0, 0},
    /* ABSORB_REG    */ {H2V_ARG_NONE, H2V_ARG_REG, H2V_ARG_NONE, 1, 1, 0},
    /* ABSORB_CI     */ {H2V_ARG_NONE, H2V_ARG_NONE, H2V_ARG_NONE, 1, 1, 1},
    /* LOAD_INSTANCE */ {H2V_ARG_REG, H2V_ARG_PI, H2V_ARG_NONE, 0, 0, 0},
    /* READ_POINT    */ {H2V_ARG_NONE, H2V_ARG_OFF48, H2V_ARG_NONE, 1, 1, 0},
    /* READ_SCALAR   */ {H2V_ARG_REG, H2V_ARG_OFF32, H2V_ARG_NONE, 1, 1, 0},
    /* SQUEEZE       */ {H2V_ARG_REG, H2V_ARG_NONE, H2V_ARG_NONE, 1, 1, 0},
    /* CONST         */ {H2V_ARG_REG, H2V_ARG_CONST, H2V_ARG_NONE, 0, 0, 0},
    /* ADD           */ {H2V_ARG_REG, H2V_ARG_REG, H2V_ARG_REG, 0, 0, 0},
    /* SUB           */ {H2V_ARG_REG, H2V_ARG_REG, H2V_ARG_REG, 0, 0, 0},
    /* MUL           */ {H2V_ARG_REG, H2V_ARG_REG, H2V_ARG_REG, 0, 0, 0},
    /* NEG           */ {H2V_ARG_REG, H2V_ARG_REG, H2V_ARG_NONE, 0, 0, 0},
    /* INV           */ {H2V_ARG_REG, H2V_ARG_REG, H2V_ARG_NONE, 0, 0, 0},
    /* OUT_SCALAR    */ {H2V_ARG_TERM, H2V_ARG_REG, H2V_ARG_NONE, 0, 0, 0},
    /* ASSERT_ZERO   */ {H2V_ARG_NONE, H2V_ARG_REG, H2V_ARG_NONE, 0, 0, 0},
    /* NOP           */ {H2V_ARG_NONE, H2V_ARG_NONE, H2V_ARG_NONE, 0, 0, 0},
};
static_assert(H2V_OP_END == 0 && H2V_OP_SQUEEZE == 6 && H2V_OP_MUL == 10 && H2V_OP_OUT_SCALAR == 13 && H2V_OP_NOP == 15 && H2V_OP_COUNT == 16,
              "the rows of H2V_OPS stand in the order of the opcodes");
static constexpr bool h2v_op_known(int op) { return op >= 0 && op < H2V_OP_COUNT; }
static constexpr bool h2v_op_reads_a(int op) { return h2v_op_known(op) && H2V_OPS[op].a == H2V_ARG_REG; }
static constexpr bool h2v_op_reads_b(int op) { return h2v_op_known(op) && H2V_OPS[op].b == H2V_ARG_REG; }
static constexpr bool h2v_op_writes(int op) { return h2v_op_known(op) && H2V_OPS[op].dst == H2V_ARG_REG; }
static constexpr bool h2v_op_transcript(int op) { return h2v_op_known(op) && H2V_OPS[op].transcript; }

// LDS left for the combiner's register file in a block: 160 KB minus the 8 KB hash buffer and 1 KB of slack (plan.py:
// VM_LDS_BYTES), and THE rule by which a program of n_regs registers on `lanes` lanes per proof fits it: a block is one wave
// of 64 / lanes proofs, each register 32 bytes (lanes >= 1).
#define H2V_VM_LDS_BYTES ((size_t)160 * 1024 - 8192 - 1024)
static constexpr bool vm_fits_lds(uint32_t n_regs, uint32_t lanes) { return (size_t)n_regs * 32 * (64 / lanes) <= H2V_VM_LDS_BYTES; }

enum { H2V_TERM_PROOF_POINT = 0, H2V_TERM_VK_BASE = 1, H2V_TERM_COMMITTED_INSTANCE = 2, H2V_TERM_ACC_POINT = 3 };

// per-proof status bits produced on the device: H2V_ST_* of include/h2v.h (0 = nothing wrong so far)
#ifndef H2V_ST_BAD_SCALAR
#define H2V_ST_BAD_SCALAR 1u
#define H2V_ST_INVERSE_OF_ZERO 2u
#define H2V_ST_SHORT_PROOF 4u
#define H2V_ST_BAD_POINT 8u
#define H2V_ST_PAIRING 16u
#endif
#ifndef H2V_ST_RECURSION
#define H2V_ST_RECURSION 32u
#endif

struct H2vInstr {
    uint8_t op, pad;
    uint16_t dst, a, b;
};

// device view of a loaded plan (all pointers are device pointers)
struct H2vDevPlan {
    uint32_t proof_len, n_pi, n_ci, n_regs, n_instr, n_consts, n_points, n_vk_bases, n_terms, n_trace, pi_point;
    uint32_t vm_lanes;         // records per bundle of `instr` (the launcher swaps in the wide schedule's instr / n_instr / n_regs / vm_lanes)
    const H2vInstr *instr;
    const uint32_t *consts;    // n_consts * 8   (Fr, Montgomery)
    const uint32_t *points;    // n_points       (byte offset in the proof)
    const uint32_t *vk_bases;  // n_vk_bases * 24 (affine x||y, Montgomery; all-zero = infinity)
    const uint32_t *terms;     // n_terms * 2    (kind, index)
    const uint32_t *lines_sg2; // 68 * 48        (lambda.c0, lambda.c1, c.c0, c.c1)
    const uint32_t *lines_g2;
    const uint32_t *lines28_sg2; // 68 * 8 operand slots of 16 dwords (28-bit limbs): cooperative pairing engine
    const uint32_t *lines28_g2;
    // six-lane pairing engine, derived at plan load from the two tables above (not part of the blob): per line both loops'
    // unit-coefficient constants [A0, A1, B0, B1] = (-lambda / c, 1 / c) as operand slots of 16 dwords, 68 x 2 x 4 of them; NULL
    // when some c is zero (the launcher then never takes that engine).  six_k: [1, K1, K2, K1 K2] (Fp2, 2 x 12 Montgomery words
    // each), K_u = the product of loop u's c along the Miller schedule - read by the probe's dump path alone.
    const uint32_t *six_norm28;
    const uint32_t *six_k;
    const uint32_t *trace;     // n_trace * 2    (slot id, register)
    // recursion (IVC): terms [0, n_main_terms) are the proof's own MSM, term n_main_terms is acc_left, the rest
    // acc_right and its fixed bases; acc_idx = public-input positions of (x_hi, x_lo, y_hi, y_lo) x (left, right)
    uint32_t ivc, n_main_terms;
    uint32_t acc_idx[8];
    const uint32_t *fold_terms;  // 4 x (kind, index): el + c*acc_left, er + c*acc_right over the fold's own point buffer
    const uint32_t *vk_tab;      // n_vk_bases x 2 x 224: affine window tables [1..8]B and [1..8]phi(B), built at plan load
    // fixed-base MSM launches (non-recursive plans whose VK-base terms are the tail of the term list): all-window tables of
    // the VK bases [base][65][8][28]; terms [0, n_var) are per-proof points, [n_var, n_var + n_fix) VK bases
    const uint32_t *fix_tab;
    uint32_t n_var, n_fix;
    // window width of the all-window tables (4, 8 or 12 bits: signed digits, 2^(c-1) entries per window) and their number
    // of windows W; layout fix_tab[base][W][2^(c-1)][28] (affine x, y: 2 x 14 limbs of 28 bits)
    uint32_t fix_c, fix_W;
    // optional wide schedule of the program (0 lanes = none); host-side use only (launch_vm swaps it in)
    uint32_t wide_lanes, wide_n_regs, wide_n_instr;
    const H2vInstr *wide_instr;
    // transcript hash of the key.  tr_kind picks the combiner's instantiation on the host (launch_vm); the Cardano
    // instantiation reads none of these.  For the keyed blake2b-512 flavour the hash state every proof starts from is
    // worked out once at plan load (h2v_hostmath.hpp: b2_compress_host): tr_h0 = the parameter block's state after the
    // key block, tr_t0 = bytes compressed so far (128 with a key, 0 without: then tr_h0 is the plain initial state).
    uint32_t tr_kind, tr_t0;
    uint64_t tr_h0[8];
};
// per-proof point slots: the proof's G1 elements, the committed instance, then (recursion) the two accumulator points
#define H2V_SLOTS(plan) ((plan).n_points + (plan).n_ci + 2u * (plan).ivc)
