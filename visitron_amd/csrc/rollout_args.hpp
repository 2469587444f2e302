// Argument blocks of the rollout kernels (rollout.hip, lstm_persistent.hip), shared with the C-ABI layer (capi.hip).
#pragma once
#include "common.hpp"

struct LstmStepArgs {
  const float* xproj; long ldx;      // row b at xproj + b * ldx (already offset to position t), 4*hs wide
  const float* h_prev;               // [B, hs]
  float* h_out;                      // [B, hs]  (must not alias h_prev: other workgroups still read it)
  float* c;                          // [B, hs]  updated in place
  const bf16_t* w_hh;                // [4*hs, hs]
  const int* lengths;                // [B] or null (all rows active)
  float* seq_out; long ld_seq;       // optional: row b at seq_out + b * ld_seq (already offset to position t), hs wide
  int B, hs, t;
  const int* xrow_start;             // optional (compacted xproj rows): row of (b, t) = xrow_start[b] + t, xproj then
  long ldx_row;                      // points at row 0 and ldx_row is the row stride (ldx unused)
  // training (all optional, rows of an inactive position are left as the caller initialised them):
  float* sv_gates; long ld_svg;      // activated gates i, f, g, o of this step: row b at sv_gates + b * ld_svg, 4*hs wide
  float* sv_c; long ld_svc;          // the cell state BEFORE this step, hs wide
  bf16_t* sv_h; long ld_svh;         // the hidden state BEFORE this step as bf16 (the weight gradient's operand), hs wide
};

// One step of back-propagation through time for the same recurrence (lstm_step_bwd_kernel).
struct LstmBwdArgs {
  const bf16_t* dg_next; long ld_dgn;   // gate gradients of the step that consumed this step's h (row b at + b * ld), or null
  const bf16_t* w_hh_t;                 // W_hh transposed: [hs, 4*hs] bf16
  const float* dh_final;                // [B, hs] or null (zeros): gradient of the final hidden state
  const float* d_out; long ld_dout;     // gradient of the padded output at this position (row b at + b * ld) or null
  float* dc;                            // [B, hs] running cell-state gradient (initialised to the final state's), in place
  const float* sv_gates; long ld_svg;   // what the forward step saved
  const float* sv_c; long ld_svc;
  bf16_t* dg_out; long ld_dg;           // this step's gate gradients (pre-activation), 4*hs wide, zeros for inactive rows
  float* dg_out_f32; long ld_dgf;       // optional fp32 copy (the cell's dense backward reads it)
  const int* lengths;                   // [B] or null
  int B, hs, t, t_next;                 // t_next: position of dg_next (a row inactive there takes dh_final instead)
};

struct SoftDotBwdArgs {
  const float* target;          // [B, D]
  const float* context;         // [B, L, D] (strides as the forward)
  long ld_batch, ld_row;
  const unsigned char* mask;    // [B, L] or null
  const float* d_weighted;      // [B, D] or null
  const float* d_attn;          // [B, L] or null: gradient of the returned probabilities (output_prob) / masked logits
  float* d_target;              // [B, D]
  float* d_context;             // [B, L, D] contiguous, or null
  int B, L, D, output_prob;
};

struct SoftDotArgs {
  const float* target;          // [B, D], 1 <= D <= 4096
  const float* context;         // [B, L, D], row stride ld_row, batch stride ld_batch (elements, any)
  long ld_batch, ld_row;
  const unsigned char* mask;    // [B, L] (nonzero = masked) or null
  float* weighted;              // [B, D] or null
  float* attn;                  // [B, L] or null: probabilities (output_prob) or the masked logits
  int B, L, D, output_prob;
};

struct SkinnyArgs {
  const float* x0; long ld0; int K0;   // [M, K0] fp32, any K0 >= 1 and row stride
  const float* x1; long ld1; int K1;   // [M, K1] fp32 or null: K-concatenated behind x0 (any K1 >= 0; a group of 4 may straddle)
  const bf16_t* w; long ldw;           // [N, Kpad] bf16, zero past K0 + K1; Kpad % 32 == 0
  const float* bias;                   // [N] or null
  float* out; long ldo;                // [M, N] fp32
  int M, N, Kpad, act;                 // act: 0 none, 2 tanh
};

// The whole recurrence as one persistent launch (lstm_persistent.hip).
struct LstmPersistArgs {
  const float* xproj; long ldx_b, ldx_t;   // padded layout: row (b, t) at xproj + b * ldx_b + t * ldx_t (xrow_start == null)
  const int* xrow_start;                   // compacted layout: row (b, t) at xproj + (xrow_start[b] + t) * ldx_t
  float* h; float* c;                      // [B, hs] fp32: initial state in, final state out
  const bf16_t* w_hh;                      // [4 hs, hs]
  const int* lengths;                      // [B] or null
  float* seq_out; long lds_b, lds_t;       // optional [B, T, hs] view
  bf16_t* xchg;                            // 2 x [hs / 16][Bp][16] bf16 exchange buffers (Bp = batch rounded up to 16)
  unsigned* sync;                          // [0] arrival counter, [1] timeout flag (zeroed by the launcher)
  int B, hs, T, reverse;
};

// The turn-based decoder's LSTM cell fused with its input projection (turn_based.hip).
struct TbCellArgs {
  const long* ids; const float* table; long ld_t; int A;   // first operand, form 1: embedding rows table[ids[b]] ([A, E] fp32)
  const float* x_emb; long ld_e;                           // form 2: a ready fp32 [B, E] block (ids == null)
  const float* feature; long ld_f;                         // [B, F] fp32
  int E, F;
  const float* h_prev;               // [B, hs] fp32, 16-byte aligned
  const float* c_prev;               // [B, hs] fp32 (may be c_out)
  const bf16_t* w_ih; long ldw;      // [4*hs, Kpad] bf16, zero past E + F; Kpad % 32 == 0
  int Kpad;
  const bf16_t* w_hh;                // [4*hs, hs] bf16
  const float* bias;                 // [4*hs] fp32 = b_ih + b_hh
  float* h_out; float* c_out;        // [B, hs] fp32 (h_out must not alias h_prev)
  float* sv_gates; float* sv_c; bf16_t* sv_h;   // optional training saves, contiguous: [B, 4*hs], [B, hs], [B, hs]
  int* err;                          // device flag raised by an id outside [0, A), or null
  int B, hs;
};

// The action head of one turn-based step (turn_based.hip).
struct TbHeadArgs {
  const float* logit; long ld;               // [B, A] fp32, A <= 64 (not modified)
  const long* target;                        // [B]
  const unsigned char* blocked; long ld_blk; // [B, A] or null: non-zero = the logit counts as -inf
  long ignore_index;
  int B, A, mode;                            // mode: 0 teacher, 1 argmax, 2 sample
  uint32_t seed;
  float* loss; float* count;                 // [1] each: mean loss over the counted rows, number of counted rows
  long* a_t;                                 // [B] next action (optional for mode 0)
  int* err;                                  // device flag raised by a target outside [0, A) that is not ignore_index
};

struct TbHeadBwdArgs {
  const float* logit; long ld;
  const long* target;
  const unsigned char* blocked; long ld_blk;
  long ignore_index;
  int B, A;
  const float* g; const float* count;        // [1] each, on the device: gradient of the loss, the forward's count
  float* dlogit; long ld_d;                  // [B, A] fp32
};

// The rollout's observation tensors gathered from the device feature store (observations.hip).
struct ObsGatherArgs {
  const float* store; long N; int V, D;      // [N, V, D] fp32
  const float* table;                        // [V, V, 4] fp32: [base view][view][sin h, cos h, sin e, cos e]
  const int* rows;                           // the staged record's parts: [B][3] slot, view_index, cand_count
  const int* pts;                            // [B][Cmax] candidate views
  const double* agent;                       // [B][2] heading, elevation
  const double* cand_h; const double* cand_e;   // [B][Cmax] each
  int B, Cmax;
  float* a_t; float* f_t; float* cand;       // [B, 4], [B, V, D+4], [B, Cmax, D+4]
  int* leng; unsigned char* mask;            // [B], [B, Cmax]
  int* err;                                  // device flag raised by a bad index, or null
};

struct ObsViewArgs {
  const float* store; long N; int V, D;
  const int* rows;                           // [B][2] slot, view_index
  int B;
  float* out; long ld_out;                   // [B, D] fp32
  int* err;
};
