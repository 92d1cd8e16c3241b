// The size constants of the bucket MSM (h2v_pippenger.hpp), apart from its kernels so that host-only code - the workspace's size
// tables, h2v_ws_layout.hpp - reads the same definitions.  HOST CODE ONLY: no HIP call and no HIP header in this file.
#pragma once

#define PIP_PT_DW 42          // x, y, beta*x: 3 x 14 limbs per term
#define PIP_PART_DW 44        // Jacobian partial sum: 42 limbs + infinity flag + pad (16-byte multiple)
#define PIP_MAX_W 20
#define PIP_MAX_C 10          // NB = 2^(c-1) <= 512 buckets per window: one block's LDS holds a window's bucket sums
#define PIP_N_CLASSES 9       // lanes per bucket: 2^0 .. 2^8
#define PIP_CLS_DW (3 * PIP_N_CLASSES + 1)   // per class: first rank, end rank, first lane; then the lane total
#define PIP_ARGS_BYTES 144    // sizeof(PipArgs): what one problem of a many-problem launch reads (h2v_capi.hip asserts it)
