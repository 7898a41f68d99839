/* desire_hip.h -- C ABI of libdesire_hip.so: DESIRE sample-generation + ranking/refinement hot
 * path on MI355X (gfx950).
 *
 * The reference (tdavchev/DESIRE) has NO FFI / plugin / operator interface: its hot path is
 * one Python function that unrolls a per-object loop into a TF1 graph
 * (/root/reference/model/model.py:79-403, loop at :211) behind two Python classes
 * (DESIREModel model/model.py:29, DataLoader utils/data_loader.py:20).  This ABI is therefore
 * the boundary a maintainer would bind with ctypes from model/model.py; each entry point
 * below names the reference lines whose work it replaces.  See INTEGRATION.md for the stub.
 *
 * Conventions
 *   - plain C, no torch types; every pointer named dev_* is a DEVICE pointer owned by the
 *     caller (e.g. torch tensor .data_ptr()), every pointer named host_* is host memory.
 *   - all tensors fp32, C-contiguous, layouts given per argument.
 *   - row index r = (scene*K + k)*mno + slot   (R = n_scenes*K*mno rows);
 *     agent index a = scene*mno + slot          (A = n_scenes*mno agents).
 *   - every call returns 0 on success, <0 on error; desire_last_error() gives the text.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are
 *     stream-ordered and asynchronous; one handle per device, not thread-safe per handle.
 *   - there is no CPU path: on a machine without a gfx950 device desire_create fails.
 */
#ifndef DESIRE_HIP_H
#define DESIRE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DESIRE_OK 0
#define DESIRE_ERR_ARG (-1)     /* bad argument / dims */
#define DESIRE_ERR_STATE (-2)   /* weights missing, grids missing, ... */
#define DESIRE_ERR_HIP (-3)     /* a HIP runtime call failed */
#define DESIRE_ERR_NODEV (-4)   /* no gfx950 device */

/* Mirrors desire_amd/spec.py:Dims.  Field meaning and the reference args they come from:
 * mno=max_num_obj, T_obs/T_pred (ref: one seq_length), H=d_dim, L=latent_size,
 * S=int(sqrt(2*rnn_size)) (model/model.py:44-60); grid_size (train.py:71-72);
 * nb_w/nb_h = neighborhood_size (train.py:68-70) in normalised units; sx/sy pixel scale. */
typedef struct desire_dims {
    int32_t n_scenes, mno, K, T_obs, T_pred;
    int32_t H, L, S, C, Gh, Gw, n_grids;
    int32_t grid_size, E_v, iters, posterior;
    float nb_w, nb_h, sx, sy;
    int32_t bin_mode;      /* social pooling layout: 0 = rectangular grid_size x grid_size window of nb_w x nb_h (Social-LSTM /
                              the reference's flags, train.py:68-72); 1 = log-polar (the paper's): grid_size rings with
                              geometric radii between nb_h (inner radius) and nb_w (outer radius) x grid_size sectors */
    int32_t bn_mode;       /* batch normalisation of the CVAE conv stacks: 0 = frozen moving statistics folded into the kernels
                              (default); 1 = "per-object": the reference's literal graph -- phase=train on a batch of one
                              object (model/model.py:453-462,471-481), i.e. per-sample per-channel moments over the layer's
                              pixels.  2 = whole-batch statistics: the same phase=train moments taken over everything one call
                              batches (per channel over all samples and pixels) -- what prettytensor's default does when objects ARE
                              batched.  Modes 1 and 2: fp32 operands; mode 1 also trains (desire_backward goes through the per-sample
                              normalisation); mode 2 trains too (desire_backward takes the gradient means over every sample of the call; with
                              several data-parallel ranks each rank normalises over ITS share of the batch). */
    int32_t bf16;          /* 0: fp32 matrix operands (default); 1: bf16 operands / fp32 accumulate + fp32 state
                              for the recurrent IOC kernel (BASELINE configs[2]); inference only.  2: SPLIT bf16 operands --
                              every fp32 operand enters the bf16 matrix pipe as hi + lo (hi = bf16(x), lo = bf16(x - hi)) and a
                              product is three bf16 MFMAs (hi.hi + lo.hi + hi.lo, fp32 accumulate): results agree with the fp32
                              kernels to ~1e-5 relative at 3/16 of their matrix time: the IOC kernel, and in a training step the IOC
                              BPTT, the large weight-gradient reductions and data-gradient convolutions (gradients stay within 2e-4 of
                              float64 autograd); sample generation (decoder, deconv2, deconv3) runs the six-product kernels of mode 3,
                              because two-piece operands there would move the sampled positions.  Kernels without a split form run the
                              fp32 kernels, so 2 is always at least as accurate as it claims.  3: THREE bf16 pieces per operand
                              (x = hi + mid + lo exactly) and six products per fp32 product -- every term down to 2^-16 |a b| -- i.e.
                              the accuracy class of the fp32 fmaf chain itself at 6/16 of its matrix time; inference only, same
                              shapes as 2 (others run the fp32 kernels). */
    int32_t ref_compat;    /* 1: the reference graph AS WRITTEN (model/model.py:116-311) instead of the frozen spec: the GRU
                              decoder runs n_dec steps (7, :280) and every output state [H] is re-read as T_obs (x, y) points
                              (:286-289, needs H == 2*T_obs); one eps per object (K = 1, :262-263); target window = input
                              shifted one frame (T_pred == T_obs, utils/data_loader.py:206-207); per-object batch-norm
                              (bn_mode = 1); no head, no IOC (:312-313).  desire_sample / desire_forward then write
                              dev_Yhat [A, n_dec, T_obs, 2] = output_states; desire_ioc_refine is an error.  sx = sy = 1
                              reproduces the raw-pixel inputs of :216-231. */
    int32_t n_dec;         /* ref_compat only: decoder steps (the reference hard-codes 7); 0 otherwise */
    /* ---- behavioural switches (round 4: these were environment variables read inside the library; a C caller could neither see nor
     * set them).  All zero = the measured winners.  desire_set_option changes them on a live handle. ---- */
    int32_t ioc_form;      /* which form of the IOC kernel serves the shape: DESIRE_IOC_* below.  Every form computes the same function;
                              forms differ in fp32 summation order only (<= 2e-6 on trajectories), except DESIRE_IOC_COMPACT, which also
                              executes fewer products (exact zeros skipped). */
    int32_t ioc_split;     /* the BIN-SPLIT regime of the fp32 inference IOC kernel.  A call with few 32-row tiles (tiles * n <= the
                              workgroups the device keeps resident, n = 2..4) spreads the social bins of every tile over n workgroups that
                              exchange partial sums once per step: one window 3.5 -> 2.4 ms.  CONSEQUENCE: with the default (0 = auto)
                              the fp32 result of a window depends on HOW MANY windows share the call -- the partial sums of the social
                              embedding are regrouped, a difference of <= 2e-6 in trajectories and scores (inside every gate of
                              tests/, but not bit-identical across batch sizes).  1 = never split: results of a window are bit-identical
                              whatever the batch (the rounds 1-2 behaviour).  n > 1 = at most n workgroups per tile. */
    int32_t train_fp32_mask; /* dims.bf16 = 2 training step: bit mask of the parts that stay on fp32 operands instead of split-bf16 ones
                              (1 weight-gradient reductions, 2 data-gradient convolutions, 4 IOC BPTT, 8 six-product sample generation
                              in the forward pass); 0 = everything that has a split form uses it. */
    int32_t flags;         /* DESIRE_FLAG_* below */
} desire_dims;

#define DESIRE_IOC_AUTO 0          /* the measured winner per shape */
#define DESIRE_IOC_TILE64 2        /* 64-row tiles also for groups of <= 32 agents (fp32 and bf16 operands) */
#define DESIRE_IOC_CLUSTER 4       /* groups of 64 agents through the cluster form (one group = two workgroups exchanging hidden states
                                      through global memory; the default for 96 / 128 agents); bf16 operands: with column-split pooling */
#define DESIRE_IOC_CLUSTER_BINS 6  /* bf16 operands, 64 agents: the cluster form with the pooling split over bins (what 96 / 128 run) */
#define DESIRE_IOC_COMPACT 8       /* row-compacted social pooling (fp32 inference, groups of <= 32 agents, H <= 128): the pooling MFMAs
                                      run on the rows that have a neighbour in the bin only */
#define DESIRE_IOC_TRAIN_DENSE 9   /* training-mode forward with the dense pooling (default there: the compacted one) */
#define DESIRE_IOC_X6_TILE32 13    /* dims.bf16 = 3: the 32-row / three-image six-product kernel whatever the launch size */
#define DESIRE_IOC_X6_TILE64 14    /* dims.bf16 = 3: the 64-row six-product kernel whatever the launch size (default: launches of >= 256 tiles) */
#define DESIRE_FLAG_NO_FUSE34 1    /* dims.bf16 = 1: deconv3 and deconv4 as separate kernels (default: fused, d3 never written) */
#define DESIRE_FLAG_TRAIN_FWD_3P 2 /* dims.bf16 = 2, training mode: the forward pass's sample generation (GRU decoder, deconv2, deconv3) with TWO-piece
                                      operands (three bf16 products per fp32 product, the first two pieces of the same packs) instead of three pieces /
                                      six products: 67.6 instead of 70.0 ms per 81 920-sample step, every weight gradient within 5e-4 of float64
                                      autograd instead of 2e-4 (Y0 moves by ~1e-5, and the step's rounding class becomes that of the IOC kernels) */

#define DESIRE_FLAG_COMPACT_ROWS 4  /* PRESENT-ROW COMPACTION.  The loader pads every window to max_num_obj slots (utils/data_loader.py:209-229) and the reference
                                      masks id-0 objects in the cost only (model/model.py:351-366); with this bit the per-row sample-generation stages
                                      (reparameterisation, deconv1..4, mask fc, GRU decoder -- and in training their saves and their whole backward) run on
                                      the K rows of the agents PRESENT at the last observed frame only.  Rows of present agents are bit-identical to the
                                      uncompacted path (every stage is row-independent); the GRU encoders and the CVAE encoder run on the present agents too (their
                                      windows gathered into one pseudo-scene; "Hx" / "Hy" / "z_mean" of absent agents read back as zeros; not while
                                      desire_set_head_loss is on, whose term also counts objects that left before the last observed frame); rows of absent
                                      agents come back as zeros in dev_Yhat / "Y0" instead
                                      of the decode of an all-zero track.  The IOC stage keeps its scene-shaped tiles.  COUNTS: in inference with frozen
                                      batch-norm (bn_mode 0) the host never learns how many agents are present -- every compacted launch is sized for the
                                      worst case and reads its count from a device word the scan kernels wrote (round 6), so there is NO host wait and a compacted
                                      desire_forward can be captured in a hipGraph and replayed on other data.  In training, with bn_mode 1, or after
                                      desire_set_option(h, "compact_host_counts", 1) the count is read back through a mapped word instead (one host wait per
                                      desire_encode, launches sized exactly, not capturable).  Not with bn_mode = 2 (whole-batch statistics would
                                      change) or ref_compat.  The intermediates "vae_in", "z", "d1".."d3", "xhat", "xz" of desire_read_buffer are then in the COMPACT
                                      row order r' = k*P + a' (P = present agents, a' = rank of the agent among them). */

#define DESIRE_FLAG_COMPACT_IOC 8   /* IOC SLOT CLASSES.  The IOC kernels tile rows by whole (scene, k) groups of mno slots, so a window with 9 of 32 slots present
                                      still costs 32 rows per sample.  With this bit every window is re-seated in the smallest slot class m in {8, 10, 16, 32, 64, 96 (the three largest below mno; 10 = three groups per padded 32-row tile, where the padded-tile kernels serve the handle: inference, fp32 or split operands, H <= 128), mno}
                                      that holds its present agents (compacted to the front, order kept), the windows of a class run as one pseudo-batch on the
                                      same kernels, and windows without a present agent are not run (their dev_Yhat rows are left as they came, score 0); rows of
                                      absent agents inside a window likewise keep their incoming dev_Yhat and get score 0.  A class too small to fill the device
                                      (< 8192 rows) is folded into the next larger one, so -- like dims.ioc_split -- the summation order of a window's social
                                      pooling, i.e. the last bits of its result (<= 2e-6 on trajectories), depends on what else is in the batch.  Counts as for
                                      DESIRE_FLAG_COMPACT_ROWS (device-side in inference: every class is launched for the worst case at a static offset of the
                                      class buffers and an empty class's grids exit); shapes on the step-wise IOC (mno > 128; split operands at H = 256)
                                      ignore the bit. */

typedef struct desire_ctx desire_handle;

const char* desire_last_error(void);
int desire_version(void);
/* sizeof(desire_dims) as THIS library was built: a host compiled against another revision of this header (the struct has grown by appending
 * fields) compares it with its own sizeof before the first desire_create and refuses to run on a mismatch. */
int desire_dims_size(void);
/* First 16 hex digits of the sha256 over every source file under csrc, this header and the compile flags the library was built from (desire_amd/_build.py:
 * source_hash): equal to the tree's value <=> the loaded .so is the tree's code.  "unstamped" for a build that bypassed _build.py. */
const char* desire_build_hash(void);
/* Changes one of the behavioural switches of desire_dims on a live handle: name = "ioc_form", "ioc_split", "train_fp32_mask" or
 * "flags"; takes effect at the next call (a flag that changes what desire_encode prepares -- DESIRE_FLAG_COMPACT_* -- at the next
 * desire_encode).  "compact_min_rows" (not a desire_dims field): the fold threshold of DESIRE_FLAG_COMPACT_IOC.  "compact_host_counts" (not a
 * desire_dims field): 1 = inference reads the compaction counts back like training does (see DESIRE_FLAG_COMPACT_ROWS), 0 = device-side counts (default).
 * "scene_grad" (not a desire_dims field): 1 = desire_backward also writes d loss / d grids [n_grids, Gh, Gw, C] of the grids desire_set_scene_grids
 * gave into the workspace tensor "scene_grid_grad" (desire_device_buffer; bitwise reproducible, no weight gradient changes); 0 = off (default), and
 * the tensor is then refused (DESIRE_ERR_STATE), as it is outside training mode.
 * Unknown name or value out of range: DESIRE_ERR_ARG. */
int desire_set_option(desire_handle* h, const char* name, int32_t value);

/* Replaces DESIREModel.__init__/build_model graph construction (model/model.py:36-77). */
int desire_create(const desire_dims* dims, desire_handle** out);
int desire_destroy(desire_handle* h);

/* Weights by name (names/shapes: desire_amd/spec.py:weight_shapes; the reference's own names
 * are define_weights model/model.py:420-451 plus the implicit TF/prettytensor scopes).
 * host_data is n fp32 values in the natural (TF) layout; the library repacks GEMM operands
 * into MFMA B-fragment order and uploads.  desire_finalize_weights folds frozen batch-norm
 * (model/model.py:457-462) into per-channel scale/shift and verifies every tensor is set. */
int desire_set_weight(desire_handle* h, const char* name, const float* host_data, size_t n);
int desire_finalize_weights(desire_handle* h);

/* Scene feature grids rho(I) (absent in the reference, model/model.py:312-313; the `grid`
 * argument of sample(), :613).  dev_grids [n_grids, Gh, Gw, C]; host_grid_of_scene [n_scenes].
 * The device buffer is referenced, not copied: keep it alive while the handle uses it. */
int desire_set_scene_grids(desire_handle* h, const float* dev_grids, const int32_t* host_grid_of_scene);
/* Scene IMAGES instead of precomputed grids: dev_images [n_grids, Hi = 4*Gh, Wi = 4*Gw, 3] (referenced, not copied: keep it alive), host_grid_of_scene
 * [n_scenes] validated as above.  The handle then owns its grid buffer and runs the scene CNN of desire_scene_cnn itself (bit-identical grid): a
 * training-mode desire_forward every step, keeping the post-ReLU activations; an inference-mode forward only when the grid is stale (desire_set_weight,
 * desire_finalize_weights, desire_adam_step, or the images set again).  In training, desire_backward then also fills the gradients of the six scene_cnn weights
 * (and "scene_grid_grad", as desire_set_option(h, "scene_grad", 1) does).  The last of desire_set_scene_grids / desire_set_scene_images called wins. */
int desire_set_scene_images(desire_handle* h, const float* dev_images, int32_t Hi, int32_t Wi, const int32_t* host_grid_of_scene);

/* Encoders + CVAE encoder (model/model.py:233-259,471-492).
 * dev_past [n_scenes, T_obs, mno, 3] and dev_fut [n_scenes, T_pred, mno, 3] are stacks of the
 * loader's windows (id, x_px, y_px; utils/data_loader.py:212-229).  dev_fut may be NULL when
 * dims.posterior == 0. */
int desire_encode(desire_handle* h, const float* dev_past, const float* dev_fut, void* stream);

/* Reparameterise + CVAE decoder + mask fc + GRU decoder (model/model.py:260-289).
 * dev_eps [R, L]; dev_Yhat [R, T_pred, 2] out (normalised coordinates).  dev_eps may be NULL after desire_set_rng: the call then draws its
 * eps on the device (one draw per call; see "device generator" below). */
int desire_sample(desire_handle* h, const float* dev_eps, float* dev_Yhat, void* stream);

/* IOC scoring + regression refinement, dims.iters passes (paper; model/model.py:312-313).
 * dev_Yhat [R, T_pred, 2] in/out; dev_score [R] out.  Scenes of up to 32 agents: one persistent workgroup per 32-row tile; 64 / 96 /
 * 128: the cluster form (workgroups of a group exchanging hidden states inside one launch); 160 .. 256 (mno a multiple of 32): one
 * launch per step of the agent-sharded kernel with a single rank (fp32 operands, inference only) -- same results, more launches. */
int desire_ioc_refine(desire_handle* h, float* dev_Yhat, float* dev_score, void* stream);

/* encode + sample + ioc_refine, the unit bench.py times. */
int desire_forward(desire_handle* h, const float* dev_past, const float* dev_fut, const float* dev_eps,
                   float* dev_Yhat, float* dev_score, void* stream);

/* ---- device generator: the latent noise drawn where it is consumed (csrc/philox.h, csrc/kernels_rng.hip) ----
 * Philox4x32-10 (Salmon et al., SC'11: multipliers D2511F53 / CD9E8D57, Weyl constants 9E3779B9 / BB67AE85, ten rounds), key = the 64-bit seed
 * as (lo, hi).  A 32-bit word x becomes the uniform u = ((x >> 9) + 0.5) * 2^-23 (exact in fp32, never 0 or 1); Box-Muller on the word pairs
 * (x0, x1) and (x2, x3) -- r = sqrtf(-2 logf(u1)), t = 2 pi u2, normals r cosf(t) and r sinf(t) -- makes four normals of one block, |n| <= 5.77.
 * THE COUNTERS ARE PART OF THIS CONTRACT (tests/rng_reference.py restates them in numpy, bit for bit):
 *     word   latent eps                                fill op (desire_rng_fill, kinds BITS / NORMAL)     head rollout (desire_rollout_samples)
 *     c0     (l >> 2) | slot << 10 | k << 19           low word of the block index                        (t >> 1) | slot << 10 | k << 19
 *     c1     scene_base + scene   (modulo 2^32)        high word of the block index                       scene_base + scene   (modulo 2^32)
 *     c2     draw                                      the caller's stream_id                             draw
 *     c3     0                                         1                                                  2
 * Latent l of sample k of (window scene_base + scene, slot slot_base + slot) in draw `draw` is normal l & 3 of that block (L % 8 == 0: whole
 * blocks); element e of a fill stream is word / normal e & 3 of block e >> 2.  The packing holds L <= 4096, slot_base + mno <= 512 and K < 8192.
 * Step t of rollout k of (window scene_base + scene, slot slot_base + slot) in draw `draw` takes normals 2 (t & 1) (the x draw) and 2 (t & 1) + 1 (the
 * y draw) of its block, so one block serves two steps; that packing holds T_pred <= 2048 on top of the slot and K limits.
 * So a window's noise does not depend on its position in the batch, the batch size, the rank count, the padding width or DESIRE_FLAG_COMPACT_*.
 *
 * desire_set_rng switches the generator on, or re-seeds it: next draw = `draw`.  The first call allocates four device words (next, used, seed);
 * every call sets them with one kernel, stream-ordered and capturable (the first call is not).  Afterwards dev_eps == NULL is legal in
 * desire_sample, desire_forward and desire_backward (before: DESIRE_ERR_ARG, as ever).  A sampling call with NULL eps does, ON THE DEVICE,
 * used = next; next += 1, and draws with `used` -- a replayed hipGraph therefore advances by itself, and setting the words again replays the
 * same noise.  desire_backward(NULL) regenerates the eps of `used` and does not advance: a training step keeps no eps.  A non-NULL dev_eps takes
 * the kernels it always took and leaves the counter alone.  Dims outside the packing: DESIRE_ERR_ARG. */
int desire_set_rng(desire_handle* h, uint64_t seed, uint32_t draw, void* stream);
/* The global index of the call's first window and of the handle's first slot (an agent-sharded handle whose mno is a shard).  Host-side values,
 * passed to the kernels as ARGUMENTS: a captured graph keeps the origin it was captured with.  Default (0, 0). */
int desire_set_rng_origin(desire_handle* h, uint32_t scene_base, uint32_t slot_base);
/* host_out[0] = next (the draw the next sampling call will use), host_out[1] = used (the draw of the last one).  Synchronises the stream. */
int desire_rng_state(desire_handle* h, uint32_t host_out[2], void* stream);
#define DESIRE_RNG_BITS 0     /* dev_out: n uint32, the raw stream */
#define DESIRE_RNG_NORMAL 1   /* dev_out: n fp32 normals */
#define DESIRE_RNG_LATENT 2   /* dev_out: fp32 [n_scenes, K, mno, L] = exactly the eps a NULL-eps call of this handle uses in draw `stream_id` with key
                                 `seed` at the handle's current origin; first must be 0 and n = R * L.  For tests, and for keeping a draw. */
#define DESIRE_RNG_ROLLOUT 3  /* dev_out: fp32 [n_scenes, K, mno, T_pred, 2] = exactly the normals a NULL-normals desire_rollout_samples of this handle uses in
                                 draw `stream_id` with key `seed` at the handle's current origin; first must be 0 and n = R * T_pred * 2. */
/* Stand-alone fill: dev_out[i] = element first + i of the stream (seed, stream_id), so a fill equals the matching slice of any longer one.
 * Needs no desire_set_rng and does not touch the draw counter.  Callers of desire_rollout / desire_gaussian_sample, which keep taking
 * dev_normals, fill them with kind DESIRE_RNG_NORMAL (desire_rollout_samples draws its own: see there).  Stream-ordered, capturable. */
int desire_rng_fill(desire_handle* h, uint64_t seed, uint32_t stream_id, uint64_t first, int32_t kind, void* dev_out, size_t n, void* stream);

/* Intermediates kept in the handle's workspace, for parity tests:
 * "Hx" [A,H], "Hy" [A,H], "vae_in" [A,V], "z_mean" [A,L], "z_log_sigma_sq" [A,L], "z" [R,L],
 * "d1" [R,2048], "d2" [R,4096], "d3" [R,8192], "xhat" [R,1024], "xz" [R,H], "Y0" [R,T_pred,2].
 * Any other name is looked up among the handle's internal workspace buffers (training-mode saves and gradient streams, e.g.
 * "ioc_sv_h" [R,T_pred,H]; layouts as in csrc/train.hip) -- a debugging aid, not a stable interface.
 * Copies n floats to host_out after synchronising the stream. */
int desire_read_buffer(desire_handle* h, const char* name, float* host_out, size_t n, void* stream);

/* Integer paths, exposed for bit-exact tests (the same device functions the IOC kernel uses).
 * dev_pos [n_groups, mno, 2] normalised; dev_valid [n_groups, mno] uint8;
 * dev_bins [n_groups, mno, mno] int32 out (-1 = not pooled). */
/* The log-polar bin table of a bin_mode = 1 handle: out[0..grid_size-1] squared ring radii, out[8+2k], out[9+2k] = (cos, sin)
 * of sector boundary k -- the exact fp32 constants the kernels compare against (the oracle takes them as input). */
int desire_get_bin_table(desire_handle* h, float* host_out20);
int desire_neighbor_bins(desire_handle* h, const float* dev_pos, const uint8_t* dev_valid,
                         int32_t* dev_bins, int32_t n_groups, void* stream);
/* dev_pos [n, 2] -> dev_cells [n, 2] = (cy, cx). */
int desire_scene_cells(desire_handle* h, const float* dev_pos, int32_t* dev_cells, int32_t n, void* stream);

/* Scene-context CNN rho(I) (paper; the reference has no image input, model/model.py:312-313):
 * dev_image [n_grids, Hi=4*Gh, Wi=4*Gw, 3] -> dev_grids [n_grids, Gh, Gw, C] (then pass dev_grids to
 * desire_set_scene_grids).  conv5x5/16/s2+ReLU, conv5x5/32/s2+ReLU, conv5x5/C/s1, TF SAME padding. */
int desire_scene_cnn(desire_handle* h, const float* dev_image, int32_t Hi, int32_t Wi, float* dev_grids, void* stream);

/* Train-path scalars after desire_forward (posterior mode): dev_kld [A] (model/model.py:587-589 per agent),
 * dev_recon [A] = mean_k mean_{t present} ||Y_gt - Yhat_k|| (paper; the reference's NLL has undefined inputs, :342),
 * dev_cost [2] = {mean of recon+kld over the agents that count, #such agents}.  Masking rule of :351-366,374-376: an object
 * counts when it exists (id != 0 at the last observed frame) and exists in the target; with a multi-frame target that is
 * per frame -- a target frame whose id is 0 carries no ground truth and is skipped, an object absent from every target
 * frame does not count at all.  The training loss, its gradients and desire_ade_fde use the same rule. */
int desire_losses(desire_handle* h, const float* dev_fut, const float* dev_Yhat, float* dev_kld, float* dev_recon,
                  float* dev_cost, void* stream);

/* The reference's temporal convolution O1 (model/model.py:116-133; channels are (id, x), its quirk) ->
 * dev_rho [A, 200], and feature pooling O11 (:291-311) -> dev_out [R, T_pred, 200].  No consumer exists in
 * the reference; exposed as ops for callers that want the literal tensors. */
int desire_temporal_conv(desire_handle* h, const float* dev_past, float* dev_rho, void* stream);
int desire_feature_pooling(desire_handle* h, const float* dev_Yhat, const float* dev_rho, float* dev_out, void* stream);

/* ---- rows "next" of the scope table ----
 * N1: device-side window + slot builder = DataLoader.next_batch's inner loop (utils/data_loader.py:203-229).
 * dev_frames [n_frames, mno_in, 3] is one preprocessed video (frames_from_csv layout); host_starts[i] is the
 * first frame of window i; each window spans T_obs+T_pred consecutive frames; slot = rank of the id among the
 * window's sorted unique ids (np.unique semantics, 0 included when padding exists).  Outputs
 * dev_past [n_windows, T_obs, mno, 3], dev_fut [n_windows, T_pred, mno, 3].  Returns DESIRE_ERR_ARG where the
 * reference raises IndexError (:227: more unique ids than slots) or ValueError (:224-229: an id twice in one frame).
 * Synchronises the stream (error word read-back). */
int desire_build_windows(desire_handle* h, const float* dev_frames, int32_t n_frames, int32_t mno_in,
                         const int32_t* host_starts, int32_t n_windows, float* dev_past, float* dev_fut, void* stream);
/* The same with lookahead = 1: the slots are ranked over ONE MORE frame (f0 + T_obs + T_pred, when the video has it), which is
 * what DataLoader(seq_length = T_obs + T_pred).next_batch does -- it takes np.unique over seq_length + 1 frames because its target
 * is the window shifted by a frame (utils/data_loader.py:203-209) -- so the device windows equal the x of that loader exactly,
 * including its IndexError / ValueError conditions on the extra frame.  lookahead = 0 is desire_build_windows (= a loader with
 * seq_length = T_obs + T_pred - 1, x plus the last target frame). */
int desire_build_windows_la(desire_handle* h, const float* dev_frames, int32_t n_frames, int32_t mno_in,
                          const int32_t* host_starts, int32_t n_windows, int32_t lookahead, float* dev_past, float* dev_fut, void* stream);
/* N3: bivariate-Gaussian head of sample() (model/model.py:552-565,595-611,661-669): dev_params [n,5] raw head
 * outputs, dev_normals [n,2] ~ N(0,1); dev_out [n,2] sample clipped to <= 1.0. */
int desire_gaussian_sample(desire_handle* h, const float* dev_params, const float* dev_normals, float* dev_out,
                           int32_t n, void* stream);
/* N3: sample()'s autoregressive rollout (model/model.py:623-688) in one launch: warm-up over dev_past [n_scenes, T_obs, mno, 3]
 * with the X-encoder GRU (the loop :623-632), then `num` prediction steps: the 5-wide output layer "gauss_head/w|b"
 * (the reference's output_w / output_b, :315-321,445-449) reads (mux, muy, log sx, log sy, corr) off the state, a position is
 * drawn from that bivariate Gaussian with the caller's dev_normals [num, A, 2] (:661-665), clipped to <= 1.0 (:666-669) and fed
 * back as the next input (:680-681).  dev_out [num, A, 2], normalised units.  Objects with id 0 are stepped like any other
 * (the reference does the same and carries the id over, :680). */
int desire_rollout(desire_handle* h, const float* dev_past, const float* dev_normals, int32_t num, float* dev_out, void* stream);
/* K of those rollouts per agent in ONE launch, written in the sample layout, so that everything that takes desire_sample's dev_Yhat takes this one
 * too (desire_ioc_refine, desire_rank_samples, desire_ranked_errors, desire_ade_fde).  dev_past [n_scenes, T_obs, mno, 3] as above; dev_Yhat
 * [R, T_pred, 2] out, normalised units, row r = (scene * K + k) * mno + slot; dev_normals [R, T_pred, 2] ~ N(0,1) in the same row order.  The warm-up
 * runs once per agent (into a private state buffer: "Hx" of the forward path is untouched), then T_pred steps for each of the agent's K rows: head,
 * draw, clip to <= 1.0, feed back.  Row (scene, k, slot) is the rollout desire_rollout(num = T_pred) produces for that agent from the normals of that
 * row -- the same function; the head's dot products are summed in another (fixed) order, so the last bits may differ.  A row's result does not depend
 * on the rest of the batch.  Objects with id 0 are stepped like any other; DESIRE_FLAG_COMPACT_* are ignored.  dev_normals may be NULL after
 * desire_set_rng: the normals are then computed in the kernel from the rollout counter of the device generator (one draw per call: used = next;
 * next += 1 on the device; desire_set_rng_origin applies; dims outside the packing, T_pred > 2048 among them: DESIRE_ERR_ARG), never stored;
 * desire_rng_fill(kind DESIRE_RNG_ROLLOUT) writes the same values out.  NULL normals before desire_set_rng, a NULL dev_past / dev_Yhat and a
 * ref_compat handle are DESIRE_ERR_ARG, and nothing is launched.  No host wait, no read-back; the first call allocates the state buffer, later calls
 * are capturable. */
int desire_rollout_samples(desire_handle* h, const float* dev_past, const float* dev_normals, float* dev_Yhat, void* stream);
/* N4: evaluation harness: dev_out [A,4] = (ADE mean-of-K, FDE mean-of-K, ADE best-of-K, FDE best-of-K) over the target frames
 * the object is present in (FDE: the last such frame); zeros for an object absent from every target frame. */
int desire_ade_fde(desire_handle* h, const float* dev_Yhat, const float* dev_fut, float* dev_out, void* stream);

/* ---- ranking by IOC score: the consumer of dev_score.  Agent a = scene * mno + slot, row r = (scene * K + k) * mno + slot.
 * dev_order [A, K] int32: dev_order[a, j] = the sample index k with the j-th highest score of agent a.  IEEE > on the fp32 scores; ties go to
 * the lower k (so -0.0 and 0.0 tie); NaN scores come last, among themselves by lower k; +inf first, -inf before the NaNs.  An agent whose K
 * scores are all equal -- every absent slot under DESIRE_FLAG_COMPACT_IOC -- gets the identity order, so the call needs no validity input and
 * no state of the last desire_encode.  An integer path: bit-exact.
 * Errors: frame t of agent a counts when dev_fut[scene, t, slot, 0] != 0 (desire_ade_fde's rule); e = sqrt((unit_x * dx)^2 + (unit_y * dy)^2)
 * with dx, dy as in desire_ade_fde: (unit_x, unit_y) = (1, 1) gives normalised units, (1/sx, 1/sy) pixels, (0.2/sx, 0.2/sy) the paper's 1/5
 * resolution.  For a horizon h (frames): ADE_h = mean of e over the counted frames t < h, summed in increasing t; FDE_h = e at the last counted
 * frame < h.  dev_out [A, n_h, 4] = (ADE_h, FDE_h of the sample dev_order[a, 0]; min over j < n_top of ADE_h, of FDE_h of the samples
 * dev_order[a, j]); four zeros where the agent has no counted frame before h.  With n_top = K and h = T_pred columns 2, 3 are desire_ade_fde's.
 * Neither call uses float atomics: results are bitwise reproducible and do not depend on the rest of the batch. */
/* order [A,K] int32 out (see above).  dev_top_Y [A, n_top, T_pred, 2] and dev_top_score [A, n_top] (each may be NULL): the n_top
 * best-scored samples of every agent, best first, copied from dev_Yhat / dev_score.  1 <= n_top <= K.  Stream-ordered, capturable. */
int desire_rank_samples(desire_handle* h, const float* dev_score, const float* dev_Yhat, int32_t n_top,
                        int32_t* dev_order, float* dev_top_Y, float* dev_top_score, void* stream);
/* dev_out [A, n_h, 4] (see above).  dev_order from desire_rank_samples.  host_horizons[n_h] in frames, strictly increasing,
 * 1 .. T_pred, n_h <= 8; read on the host at call time and passed by value.  Stream-ordered, capturable. */
int desire_ranked_errors(desire_handle* h, const float* dev_Yhat, const float* dev_fut, const int32_t* dev_order, int32_t n_top,
                         const int32_t* host_horizons, int32_t n_h, float unit_x, float unit_y, float* dev_out, void* stream);

/* ---- KDE log-likelihood of the ground truth under an agent's K samples: the proper scoring rule next to the best-of-n errors.  Layouts and the
 * counting rule are desire_ranked_errors': agent a = scene * mno + slot, row r_k = (scene * K + k) * mno + slot, dev_fut [n_scenes, T_pred, mno, 3],
 * frame t of agent a counts when dev_fut[scene, t, slot, 0] != 0.  dev_score [R] (the IOC scores, desire_forward's layout) or NULL.
 * All arithmetic is fp32; every operation is rounded once (no fused multiply-add), every sum over k runs in increasing k from 0.f.  For a counted
 * (a, t), with g = (fut_x * sx, fut_y * sy):
 *   1 weights     NULL dev_score: w_k = 1.f / K.  Else m = max_j s_j, e_k = expf(s_k - m), w_k = e_k / sum_j e_j -- once per agent; an agent with
 *                 any non-finite score gets 1.f / K.
 *   2 differences d_k = ((Y[r_k, t, 0] - g_x) * unit_x, (Y[r_k, t, 1] - g_y) * unit_y): the density is evaluated at the origin of the
 *                 differences, so no large coordinate enters a moment.
 *   3 mean        m = sum_k w_k * d_k.
 *   4 covariance  c_k = d_k - m; den = sum_k w_k * (1.f - w_k) (the cancellation-free form of 1 - sum w^2);
 *                 (Cxx, Cyy, Cxy) = (sum_k w_k * (c_kx * c_kx), sum_k w_k * (c_ky * c_ky), sum_k w_k * (c_kx * c_ky)) / den -- numpy's
 *                 cov(aweights = w), what scipy.stats.gaussian_kde fits.
 *   5 bandwidth   n_eff = 1.f / sum_k w_k * w_k; h2 = powf(n_eff, -1.f / 3.f): Scott's factor squared in two dimensions (scipy's default).
 *   6 degenerate  when den <= 0 (K = 1), when a weight is exactly 1.f (a one-hot score: the other weights are then below 2^-24 and the moments
 *                 above would be theirs alone), or when !(det > DESIRE_KDE_MIN_DET_RATIO * Cxx * Cyy) with det = Cxx * Cyy - Cxy * Cxy:
 *                 coincident, collinear (K = 2 among them) and non-finite samples.
 *   7 log-density q_k = (-0.5f * ((Cyy * (d_kx * d_kx) - (2.f * Cxy) * (d_kx * d_ky)) + Cxx * (d_ky * d_ky))) / (det * h2); M = max_k q_k;
 *                 l = M + logf(sum_k w_k * expf(q_k - M)) - logf(2 pi) - 0.5f * logf(det) - logf(h2), left to right.  The frame's value is l where
 *                 l > log_floor, else log_floor (a NaN among them); log_floor for a degenerate frame.  Trajectron++ clips at -20.
 *   8 outputs     dev_frame [A, T_pred] (may be NULL) = that value, 0 for a frame that is not counted.  dev_out [A, n_h, 2] = (-(sum of the frame
 *                 values over the counted t < h, in increasing t, / their number), -(the value at the last counted frame < h)); two zeros
 *                 when nothing is counted before h.
 * The density is per (unit of the caller)^2: scaling both units by c shifts every unfloored value by -2 log c.  A result depends on its agent's
 * rows, scores and targets only -- not on the grid, the batch or DESIRE_FLAG_COMPACT_*.  An absent slot's zero rows are coincident samples: it
 * reports the floor, so the call needs no validity input.  No float atomics: bitwise reproducible.  host_horizons as in desire_ranked_errors
 * (strictly increasing, 1 .. T_pred, n_h <= 8, read at call time, by value).  Stream-ordered, capturable, no host wait; the per-agent weights
 * live in scratch that desire_create allocated, a call never allocates.  K has no limit of its own.  A NULL handle / dev_Yhat / dev_fut /
 * dev_out / host_horizons, bad horizons, a non-finite log_floor, a unit that is not finite and > 0, a ref_compat handle and a T_pred beyond the
 * kernel's LDS (7680 frames): DESIRE_ERR_ARG, and nothing is launched. */
#define DESIRE_KDE_MIN_DET_RATIO 1e-5f
int desire_kde_nll(desire_handle* h, const float* dev_Yhat, const float* dev_fut, const float* dev_score, const int32_t* host_horizons,
                   int32_t n_h, float unit_x, float unit_y, float log_floor, float* dev_out, float* dev_frame, void* stream);

/* ---- n mutually distinct futures per agent: score-ordered non-maximum suppression of the K samples.  Layouts are desire_rank_samples': agent
 * a = scene * mno + slot, row r_k = (scene * K + k) * mno + slot; dev_order [A, K] int32 from desire_rank_samples (any permutation per agent: the
 * processing order); dev_score [R] or NULL.  The output dev_order_out [A, K] is again an order: desire_ranked_errors and the row gather take it
 * unchanged.  All arithmetic is fp32; every operation is rounded once (no fused multiply-add).
 *   1 distance    for samples k, k' of one agent and a frame t: a = (Y[r_k, t, 0] - Y[r_k', t, 0]) * unit_x; b = (Y[r_k, t, 1] - Y[r_k', t, 1]) * unit_y;
 *                 q_t = a * a + b * b (symmetric in k, k' bit for bit).  r2 = radius * radius.
 *   2 near        DESIRE_DIST_FINAL: q_{t_end - 1} < r2.
 *                 DESIRE_DIST_MAX:   m < r2, with m = q_0, then for t = 1 .. t_end - 1: m = q_t where q_t > m or q_t is a NaN, else m.
 *                 DESIRE_DIST_MEAN:  s / (float)t_end < radius, with s = 0.f, then for t = 0 .. t_end - 1: s = s + sqrtf(q_t).
 *                 The comparison is strict and false for a NaN: a NaN is never near.
 *   3 greedy pass for j = 0 .. K-1 the candidate is k = dev_order[a, j].  It is KEPT iff it is near no sample kept before it; otherwise it is OWNED by
 *                 the first kept sample, in keeping order, that it is near.
 *   4 order       dev_order_out[a, :] = the kept samples in keeping order, then the owned ones in processing order: a permutation whenever the
 *                 input row is one.  dev_count[a] = the number kept, >= 1.  radius == 0: nothing is near, dev_order_out == dev_order, count K.
 *                 An absent slot's zero rows coincide: for any radius > 0 its count is 1 and its order the input's -- no validity input needed.
 *   5 mass        dev_mass [A, K] (may be NULL).  The weights w are desire_kde_nll's step 1 (NULL dev_score or any non-finite score of the agent:
 *                 1.f / K; else m = max_j s_j, e_k = expf(s_k - m), w_k = e_k / sum_j e_j, sums in increasing k).  dev_mass[a, i], i < count =
 *                 the sum of w over kept sample i and the samples it owns, in processing order from 0.f; 0.f for i >= count.
 *   6 gather      dev_top_Y [A, n_top, T_pred, 2] and dev_top_score [A, n_top] (each may be NULL; dev_top_score needs dev_score): the rows / scores
 *                 of the first n_top entries of dev_order_out, as desire_rank_samples gathers them.  When count < n_top the tail is the
 *                 best-scored suppressed samples: always n_top distinct samples.
 *   7 bad indices dev_order is read only through a range check: an agent whose row holds an index outside 0 .. K-1 gets count 0, the identity
 *                 order and zero mass (its gather is the identity order's).  No case reads outside dev_Yhat.
 * A result depends on its agent's rows, order and scores only -- not on the grid, the rest of the batch, DESIRE_FLAG_COMPACT_* or the state of the
 * last desire_encode.  No atomics: bitwise reproducible.  One launch, stream-ordered, capturable, no host wait, no allocation and no scratch.
 * LDS plan: one workgroup stages the frames it walks (F = 1 for DESIRE_DIST_FINAL, else t_end) of all K samples of a chunk of slots; one agent
 * must fit: K * (8 * (F | 1) + 20) + 8 <= 61440 bytes -- e.g. (K 20, t_end 40), (K 130, t_end 9), (K 3, t_end 200), K up to 176 at t_end 40.
 * DESIRE_ERR_ARG with a desire_last_error text, and nothing is launched: a metric outside 0 .. 2; a radius that is negative or not finite; a
 * unit that is not finite and > 0; t_end outside 1 .. T_pred; n_top outside 1 .. K; a NULL dev_Yhat / dev_order / dev_order_out / dev_count;
 * dev_top_score without dev_score; a NULL handle; a ref_compat handle; a (K, t_end) beyond the LDS plan. */
#define DESIRE_DIST_FINAL 0   /* squared distance at frame t_end - 1 */
#define DESIRE_DIST_MEAN  1   /* mean over t < t_end of the per-frame distance */
#define DESIRE_DIST_MAX   2   /* largest per-frame squared distance over t < t_end */
int desire_select_diverse(desire_handle* h, const float* dev_Yhat, const int32_t* dev_order, const float* dev_score,
                          int32_t metric, int32_t t_end, float radius, float unit_x, float unit_y, int32_t n_top,
                          int32_t* dev_order_out, int32_t* dev_count, float* dev_mass,
                          float* dev_top_Y, float* dev_top_score, void* stream);

/* ---- joint (scene-level) metrics: sample k of every agent of a window was scored and refined together (the IOC stage pools over the slots of
 * one (window, k)), so the K samples of a window are K joint futures of the scene.  This call looks at them that way: does a joint future run
 * its agents through each other, what is the error of the best SCENE sample (min over k of the mean over the agents: JADE / JFDE), and which
 * joint sample does the summed score prefer.  Unless noted, layouts, the counting rule, g, the per-frame error e, ADE_h / FDE_h and
 * host_horizons are desire_ranked_errors': agent a = scene * mno + slot, row r_k = (scene * K + k) * mno + slot, dev_fut [n_scenes, T_pred, mno, 3],
 * g = (fut_x * sx, fut_y * sy) rounded once, host_horizons[n_h] strictly increasing, 1 .. T_pred, n_h <= 8, read at call time, by value.  All
 * arithmetic is fp32, every operation rounded once (no fused multiply-add); no float atomics.
 *   1 counted     exactly one of dev_fut and dev_present is non-NULL (both or neither: DESIRE_ERR_ARG).  With dev_fut: c(a, t) =
 *                 dev_fut[scene, t, slot, 0] != 0 (evaluation).  With dev_present [A] uint8: c(a, t) = dev_present[a] != 0 for every t (prediction
 *                 time, no future known); dev_jerr and dev_out must then be NULL.  A slot TAKES PART BEFORE h when it has a counted frame t < h.
 *   2 distance    for slots i != j of one (window, k) and a frame t: a = (Y[r_i, t, 0] - Y[r_j, t, 0]) * unit_x; b = (Y[r_i, t, 1] - Y[r_j, t, 1]) *
 *                 unit_y; q = a * a + b * b (symmetric in i, j bit for bit); r2 = radius * radius.  The pair TOUCHES at t iff c(i, t) && c(j, t) &&
 *                 q < r2: strict, false for a NaN; radius 0: nothing touches.
 *   3 truth       with dev_fut the same rule runs on the positions g(a, t) as a pseudo-sample k = K: the collision rate of the data under the
 *                 rule the samples are held to.
 *   4 first       dev_first [n_scenes, K + 1, mno] int32 (may be NULL) = the smallest t at which slot i touches any other slot; T_pred when there is
 *                 none, and for a slot that is never counted.  Row K is the ground truth; with dev_present it is filled with T_pred.
 *   5 counts      dev_cnt [n_scenes, K + 1, n_h, 2] int32 (required) = (slots with first < h, slots taking part before h).  The rate is the caller's
 *                 division: the library writes integers only.  With dev_present row K is all zeros (no ground truth, nobody takes part).
 *   6 errors      only with dev_fut.  dev_jerr [n_scenes, K, n_h, 2] (may be NULL) = (JADE_h, JFDE_h): the sum of ADE_h(a, k) -- of FDE_h(a, k) --
 *                 over the slots taking part before h, in increasing slot from 0.f, divided by (float) their number; zeros when no slot takes part.
 *                 ADE_h / FDE_h are the bits of desire_ranked_errors' table (the call fills it with that call's kernel and shares its scratch, so
 *                 the two calls are ordered by the stream like any two calls on one handle).
 *   7 score       dev_jscore [n_scenes, K] (may be NULL) = the sum of dev_score[r] over the slots taking part before T_pred, in increasing slot from
 *                 0.f; all zeros when dev_score is NULL.  dev_jorder [n_scenes, K] int32 (required) = the order of the window's K joint scores under
 *                 desire_rank_samples' rule exactly: IEEE >, ties to the lower k, NaNs last by index.  K has no limit of its own.
 *   8 pick        dev_out [n_scenes, n_h, 4] (may be NULL; needs dev_fut) = (JADE_h, JFDE_h of sample jorder[0]; min over j < n_top of JADE_h, and
 *                 separately of JFDE_h, over the samples jorder[j]); the minimum keeps a NaN; four zeros where nobody takes part.  1 <= n_top <= K.
 * At mno = 1 and n_top = K, dev_out is desire_ranked_errors' dev_out and dev_jorder desire_rank_samples' order wherever the slot takes part.
 * A window's results depend on that window's rows, scores and targets only -- not on the grid, the batch or DESIRE_FLAG_COMPACT_*; bitwise
 * reproducible (`first` is an integer minimum, every float sum one fixed sequence).  Stream-ordered, capturable, no host wait, no allocation: the
 * scratch was allocated by desire_create.  LDS plan: one workgroup owns one (window, k) and stages its positions as float2 [frame][slot] (frame
 * stride mno + 1 pairs from 32 slots on, mno below) next to 8 mno bytes of per-slot integers, 61440 bytes in all; when mno * T_pred positions do not
 * fit (256 slots x 40 frames = 82 KB) it walks the frames in chunks of (61440 - 8 mno) / (8 stride) frames -- 28 at 256 slots -- carrying `first`
 * across them, with the bits of an unchunked walk.  Every (mno, T_pred) of a handle is served; only dev_jerr / dev_out inherit desire_ranked_errors'
 * limit on T_pred (about 3800 frames).
 * DESIRE_ERR_ARG with a desire_last_error text, and nothing is launched or written: a NULL handle / dev_Yhat / dev_cnt / dev_jorder /
 * host_horizons; bad horizons; n_top outside 1 .. K; a radius that is negative or not finite; a unit that is not finite and > 0; both or neither
 * of dev_fut / dev_present; dev_jerr or dev_out without dev_fut; a ref_compat handle. */
int desire_joint_metrics(desire_handle* h, const float* dev_Yhat, const float* dev_fut, const uint8_t* dev_present,
                         const float* dev_score, const int32_t* host_horizons, int32_t n_h, int32_t n_top,
                         float radius, float unit_x, float unit_y,
                         int32_t* dev_first, int32_t* dev_cnt, float* dev_jerr, float* dev_jscore, int32_t* dev_jorder,
                         float* dev_out, void* stream);

/* ---- n distinct joint futures per window: score-ordered non-maximum suppression of the K WORLDS of a window, world k being sample k of every
 * slot together (what desire_joint_metrics ranks and desire_plan_risk weights).  Layouts are desire_joint_metrics': agent a = scene * mno + slot,
 * row r_k = (scene * K + k) * mno + slot.  All arithmetic is fp32; every operation is rounded once (no fused multiply-add); no float atomics.
 *   1 taking part dev_present [A] uint8 (may be NULL: every slot takes part).  Slot i takes part iff dev_present[a] != 0.  The rows of a slot that
 *                 does not take part are never read.
 *   2 per agent   for worlds k, k' of a window and a slot i: q_t, m and s are desire_select_diverse's steps 1 - 2 on the rows r_k, r_k' of slot i
 *                 (the same operation sequence, symmetric in k, k' bit for bit), near_i that call's predicate for `metric` (DESIRE_DIST_*), and
 *                 d_i the linear distance: DESIRE_DIST_FINAL sqrtf(q_{t_end - 1}); DESIRE_DIST_MAX sqrtf(m); DESIRE_DIST_MEAN s / (float)t_end.
 *   3 world       r2 = radius * radius.  DESIRE_WORLD_ALL: k and k' are NEAR iff near_i holds for every taking-part slot (a conjunction: order-
 *                 free; a NaN is never near).  DESIRE_WORLD_MEAN: D = (the sum of d_i over the taking-part slots, in increasing slot from 0.f) /
 *                 (float)(their number); NEAR iff D < radius, strict and false for a NaN.  No taking-part slot: the worlds are near whenever
 *                 radius > 0.  radius == 0: nothing is near.
 *   4 order in    the processing order of the window is the order of dev_wscore [n_scenes, K] under desire_rank_samples' rule exactly (IEEE >,
 *                 ties to the lower k, NaNs last by index), ranked by the call itself.  dev_wscore may be NULL: the identity order, uniform
 *                 weights.  Any caller-made score will do (desire_joint_metrics' dev_jscore; that minus a penalty per collision; ...).
 *   5 greedy pass desire_select_diverse's steps 3 - 4 with `sample of an agent` read as `world of a window`: dev_worder [n_scenes, K] = the kept
 *                 worlds in keeping order, then the owned ones in processing order; dev_wcount [n_scenes] = the number kept, >= 1.
 *   6 mass        dev_wmass [n_scenes, K] (may be NULL).  The weights W_k are desire_plan_risk's step 6 on dev_wscore (m = max_k, e_k =
 *                 expf(s_k - m), W_k = e_k / sum_k e_k in increasing k from 0.f; 1.f / K when dev_wscore is NULL or any score is not finite).
 *                 dev_wmass[w, i], i < count = the sum of W over kept world i and the worlds it owns, in processing order from 0.f; 0.f beyond.
 *   7 label       dev_wlabel [n_scenes, K] int32 (may be NULL): for world k the position in keeping order of the kept world that owns it, its own
 *                 position when it is kept.
 *   8 A window's result depends on that window's taking-part rows, scores and presence only -- not on the grid, the batch, DESIRE_FLAG_COMPACT_*
 *     or the last desire_encode.  Bitwise reproducible, one launch, stream-ordered, capturable, no host wait, no allocation and no scratch.
 * At mno = 1 with the slot present and DESIRE_WORLD_ALL, dev_worder / dev_wcount / dev_wmass are the bits of desire_select_diverse given
 * desire_rank_samples' order and the same scores.  With radius 0 and dev_wscore = desire_joint_metrics' dev_jscore, dev_worder is its dev_jorder.
 * LDS plan: one workgroup owns one window.  Per kept world it stages the frames it walks (F = 1 for DESIRE_DIST_FINAL, else t_end) of that world's
 * rows of a chunk of taking-part slots, next to K words per slot of the chunk, 40 K bytes of per-world words and 4 mno bytes; the candidates' rows
 * are read from dev_Yhat.  The chunks run over the slots, a world's reduction over the slots is carried across them in increasing slot: the bits
 * of an unchunked walk.  One slot must fit: 44 K + 4 mno + 8 (F | 1) <= 61440 bytes -- every (mno <= 256, T_pred <= 200) at any K <= 1300, e.g.
 * 22 slots per chunk at (mno 256, t_end 200, K 176).
 * DESIRE_ERR_ARG with a desire_last_error text, and nothing is launched or written: a NULL handle / dev_Yhat / dev_worder / dev_wcount; a metric
 * outside 0 .. 2; a reduce outside 0 .. 1; t_end outside 1 .. T_pred; a radius that is negative or not finite; a unit that is not finite and > 0;
 * a ref_compat handle; a (K, mno, t_end) beyond the LDS plan. */
#define DESIRE_WORLD_ALL  0   /* near iff every taking-part slot is near */
#define DESIRE_WORLD_MEAN 1   /* near iff the mean over the taking-part slots of the linear distance is below the radius */
int desire_select_worlds(desire_handle* h, const float* dev_Yhat, const uint8_t* dev_present, const float* dev_wscore,
                         int32_t metric, int32_t reduce, int32_t t_end, float radius, float unit_x, float unit_y,
                         int32_t* dev_worder, int32_t* dev_wcount, float* dev_wmass, int32_t* dev_wlabel, void* stream);

/* ---- candidate ego plans against the K joint futures: a planner holds M candidate trajectories for its own vehicle per window and asks of each:
 * how likely do I hit somebody before each horizon, how close do I get, when is the first contact, and which agent is the threat.  Layouts, the
 * counting rule c(a, t), g, host_horizons, radius and unit_x / unit_y are desire_joint_metrics' exactly; a slot TAKES PART BEFORE h when it has a
 * counted frame t < h.  All arithmetic is fp32, every operation rounded once (no fused multiply-add); no float atomics.
 *   1 plans       dev_plans [n_scenes, M, T_pred, 2] fp32, normalised coordinates: M >= 1 candidate ego trajectories per window.  dev_ego
 *                 [n_scenes, M] int32 (may be NULL) = the slot of the window that plan m replaces, or a negative value for none: that slot is left
 *                 out of every rule below for that plan (contact, clearance, blame); it stays in the joint score.  NULL: no plan replaces anybody.
 *                 An entry >= mno behaves as a negative one.  Exactly one of dev_fut and dev_present is non-NULL.
 *   2 distance    for plan m, slot i, joint future k and frame t: a = (P[m, t, 0] - Y[r_i, t, 0]) * unit_x; b = (P[m, t, 1] - Y[r_i, t, 1]) * unit_y;
 *                 q = a * a + b * b; r2 = radius * radius.  The plan TOUCHES slot i at t iff c(i, t) && q < r2: strict, false for a NaN (a NaN plan
 *                 frame means `the plan is not defined here` and needs no rule of its own); radius 0: nothing touches.
 *   3 truth       with dev_fut the same rule runs on the positions g(a, t) as a pseudo-sample k = K: would this plan have hit the recorded future.
 *   4 first       dev_first [n_scenes, M, K + 1] int32 (may be NULL) = the smallest t at which the plan touches any slot, T_pred when there is none.
 *                 With dev_present row K is filled with T_pred.
 *   5 clearance   dev_clear [n_scenes, M, K + 1, n_h] (may be NULL) = the minimum of q over the slots i other than the ego slot and the counted
 *                 frames t < h, starting from +inf; a NaN q never replaces the minimum, so the result does not depend on the order of the
 *                 reduction.  Squared units: the caller takes the root.  With dev_present row K is +inf.
 *   6 weights     js_k = desire_joint_metrics' step 7 (the sum of dev_score[r] over the slots taking part before T_pred, in increasing slot from
 *                 0.f: the bits of dev_jscore).  W_k is desire_kde_nll's step 1 on the K joint scores: m = max_k js_k, e_k = expf(js_k - m),
 *                 W_k = e_k / sum_k e_k, the sum in increasing k from 0.f.  W_k = 1.f / K for every k when dev_score is NULL or any js_k is not finite.
 *   7 risk        dev_risk [n_scenes, M, n_h] (required) = sum_k W_k * [first(m, k) < h] over k < K, in increasing k from 0.f.
 *   8 blame       dev_blame [n_scenes, M, n_h, mno] (may be NULL) = sum_k W_k * [plan m touches slot i at some t < h], in the same order; 0 for
 *                 the ego slot and for a slot that is never counted.
 *   9 A window's results depend on that window's rows, scores, targets and plans only -- not on the grid of workgroups, the batch, the chunks M
 *     is cut into or DESIRE_FLAG_COMPACT_*.  Bitwise reproducible (first and clearance are order-free minima, every float sum one fixed
 *     sequence), stream-ordered, capturable, no host wait, no allocation: the K weights of a window live in desire_joint_metrics' scratch of joint
 *     scores, so the two calls are ordered by the stream like any two calls on one handle.
 * LDS plan: one workgroup owns (window, chunk of PC plans), PC = as many plans as 256 (plan, slot) items hold, 32 at most, spread evenly over
 * the chunks of M.  It stages the chunk's plans as float2 [PC][frames | 1] and each unit's positions as desire_joint_metrics does, next to
 * 72 PC bytes of minima, 61440 bytes in all; when that does not fit it walks the frames in passes of (61440 - 80 PC) / (8 (PC + stride)) frames --
 * 29 at 256 slots -- carrying first and the running minimum across them, with the bits of an unchunked walk.  Every (mno, K, T_pred) of a
 * handle and every M is served.
 * DESIRE_ERR_ARG with a desire_last_error text, and nothing is launched or written: a NULL handle / dev_Yhat / dev_plans / dev_risk /
 * host_horizons; bad horizons; M < 1; a radius that is negative or not finite; a unit that is not finite and > 0; both or neither of dev_fut /
 * dev_present; a ref_compat handle. */
int desire_plan_risk(desire_handle* h, const float* dev_Yhat, const float* dev_fut, const uint8_t* dev_present,
                     const float* dev_score, const float* dev_plans, const int32_t* dev_ego, int32_t M,
                     const int32_t* host_horizons, int32_t n_h, float radius, float unit_x, float unit_y,
                     int32_t* dev_first, float* dev_clear, float* dev_risk, float* dev_blame, void* stream);

/* ---- the same, given that the ego drives the plan: desire_plan_risk weights the K joint futures by their prior weights W_k whatever the plan.
 * When plan m replaces slot e, world k also holds the model's own prediction of slot e, and the other agents of world k reacted to THAT future.
 * This call reweights the worlds of every plan by how well their ego sample agrees with the plan (importance reweighting of the joint samples
 * with a Gaussian kernel of bandwidth sigma: no model change), and reports next to the conditioned risk how well the model's prediction of the
 * ego supports the plan and how many worlds carry the answer.  Layouts, the counting rule c(a, t), g, host_horizons, radius and unit_x / unit_y
 * are desire_plan_risk's exactly, and so is everything downstream of the weights.  All arithmetic is fp32, every operation rounded once (no fused
 * multiply-add); no float atomics.
 *   C1 compared    plan m HAS AN EGO SLOT when e = dev_ego[w, m] is in 0 .. mno-1 (a NULL dev_ego, a negative entry, an entry >= mno: none).  For such
 *                  a plan frame t < t_cond is COMPARED iff c(e, t) holds and neither coordinate of P[m, t] is a NaN.  n_c = the number of compared
 *                  frames: it depends on (plan, slot) only, never on k.
 *   C2 distance    for every k < K: q_t = desire_plan_risk's step 2 between P[m, t] and row r_e of world k; S_k = the sum of q_t over the compared
 *                  frames, in increasing t from 0.f; D_k = S_k / (float)n_c, a mean squared distance in squared units.  dev_dist [n_scenes, M, K]
 *                  (may be NULL) = D_k as computed (a NaN or inf where the ego's rows are); 0.f for a plan without an ego slot or without a
 *                  compared frame.
 *   C3 logits      p_k = js_k (the bits of desire_plan_risk's step 6) when dev_score is non-NULL and every js_k of the window is finite, else 0.f.
 *                  inv = 1.f / (2.f * sigma * sigma), computed once on the host in fp32, each operation rounded, and passed by value.
 *                  l_k = p_k - D_k * inv: the product is rounded, then the difference.
 *   C4 weights     the plan is CONDITIONED iff it has an ego slot, n_c >= 1 and every l_k is finite.  Then m = max_k l_k, e_k = expf(l_k - m),
 *                  cw_k = e_k / sum_k e_k, the sum in increasing k from 0.f.  Otherwise cw_k = W_k, the bits desire_plan_risk would use.
 *                  dev_cw [n_scenes, M, K] is REQUIRED: it is the weight table the risk is summed from, so the call allocates nothing and needs no
 *                  scratch that grows with M.  dev_cond [n_scenes, M] int32 (may be NULL) = n_c for a conditioned plan, 0 otherwise.
 *   C5 ess         dev_ess [n_scenes, M] (may be NULL) = 1.f / sum_k cw_k * cw_k, in increasing k from 0.f: the effective number of worlds, 1 .. K.
 *   C6 support     dev_support [n_scenes, M] (may be NULL) = sum_k W_k * expf(-(D_k * inv)), in increasing k from 0.f; 1.f for a plan that is not
 *                  conditioned.  The unnormalised Gaussian-kernel density of the plan under the model's prediction of the ego, in (0, 1].
 *   C7 risk, blame dev_risk = desire_plan_risk's step 7 and dev_blame its step 8 with cw(m, k) in place of W_k, in the same order.  dev_first and
 *                  dev_clear do not depend on weights: desire_plan_risk's bits.  The ego slot stays out of contact, clearance and blame.
 *   C8 Step 9 of desire_plan_risk holds: a window's results depend on that window alone -- not on the grid, the batch, the chunks M is cut into or
 *      DESIRE_FLAG_COMPACT_*.  Bitwise reproducible, stream-ordered, capturable, no host wait, no allocation.  A sigma whose square overflows
 *      gives inv = 0 and therefore l_k = p_k and cw = W bit for bit wherever the D_k are finite.  Identical ego rows give cw = softmax(p).
 * LDS plan: the weights take one workgroup per (window, chunk of PC plans), PC = as many plans as 1024 (plan, k) items hold, 64 at most, spread
 * evenly over the chunks of M.  It stages the t_cond compared frames of the chunk's plans as float2 [PC][t_cond | 1] and, when the chunk's plans
 * name ONE slot and there is room (8 (PC + K) (t_cond | 1) + 8 PC <= 61440 bytes), that slot's K rows next to them (6.4 KB at K 20, T_pred 40);
 * otherwise a lane reads its world's row from dev_Yhat.  Beyond ~7600 frames of one plan the frames are walked in passes, the sums carried in
 * dev_cw, with the bits of an unchunked walk.  The K distances and numerators of a plan are parked in dev_cw itself: nothing in the LDS grows
 * with K.  The risk then runs desire_plan_risk's kernel and plan.  Every (mno, K, T_pred, M) that desire_plan_risk serves is served.
 * DESIRE_ERR_ARG with a desire_last_error text, and nothing is launched or written: everything desire_plan_risk refuses; a NULL dev_cw; a sigma
 * that is not finite or <= 0; t_cond outside 1 .. T_pred. */
int desire_plan_risk_cond(desire_handle* h, const float* dev_Yhat, const float* dev_fut, const uint8_t* dev_present,
                          const float* dev_score, const float* dev_plans, const int32_t* dev_ego, int32_t M,
                          const int32_t* host_horizons, int32_t n_h, float radius, float unit_x, float unit_y, float sigma, int32_t t_cond,
                          int32_t* dev_first, float* dev_clear, float* dev_risk, float* dev_blame,
                          float* dev_cw, float* dev_dist, float* dev_ess, float* dev_support, int32_t* dev_cond, void* stream);

/* ---- n modes with covariances per agent: what trackers, planners and the benchmark formats take -- a small mixture per agent: n modes, a
 * probability for each, a mean trajectory and a 2 x 2 covariance per frame -- fitted to the agent's K weighted samples by a weighted Lloyd
 * iteration from given seeds, and the likelihood of the ground truth under exactly that mixture.  Layouts are desire_select_diverse's: agent
 * a = scene * mno + slot, row r_k = (scene * K + k) * mno + slot; dev_order [A, K] int32 = the seed order (desire_rank_samples' output, or
 * desire_select_diverse's, which puts mutually distinct samples first); dev_score [R] or NULL; dev_fut [n_scenes, T_pred, mno, 3] or NULL (only
 * the likelihood needs it).  All arithmetic is fp32, every operation rounded once (no fused multiply-add), every sum over k or t runs in increasing
 * index from 0.f; no float atomics.
 *   1 weights     w_k = desire_kde_nll's step 1: NULL dev_score or any non-finite score of the agent: 1.f / K; else m = max_j s_j, e_k =
 *                 expf(s_k - m), w_k = e_k / sum_j e_j.
 *   2 seeds       c_i = dev_order[a, i] for i < n_modes; mean_i[t] = Y[r_{c_i}, t, :] for every t < T_pred.  Only these n_modes entries of the row
 *                 are read.  The agent is BAD when one of them lies outside 0 .. K-1 or repeats an earlier one: it gets labels -1, counts 0, prob,
 *                 mean and cov 0.f, passes 0 and log_floor at every counted frame.  No case reads outside dev_Yhat.
 *   3 distance    D(k, i) = sum over t < t_end, from 0.f in increasing t, of (a * a + b * b), with a = (Y[r_k, t, 0] - mean_i[t, 0]) * unit_x and
 *                 b = (Y[r_k, t, 1] - mean_i[t, 1]) * unit_y.
 *   4 assign      label_k: walking i = 0 .. n_modes-1, mode i is taken when D(k, i) is not a NaN and either nothing is taken yet or D(k, i) < the
 *                 distance taken (strict: ties go to the lower i; a NaN is never chosen).  Every D(k, i) a NaN: label_k = -1, and sample k is
 *                 left out of everything below.
 *   5 update      W_i = the sum of w_k over the samples with label_k = i, in increasing k from 0.f.  When W_i > 0: mean_i[t, c] = (the sum of
 *                 w_k * Y[r_k, t, c] over the same samples in the same order) / W_i for every t < T_pred.  A mode without members, or with
 *                 W_i == 0 (its members' weights underflowed), keeps the mean it has.
 *   6 iteration   labels = assign(seed means).  For p = 1 .. iters: update, assign, and stop when no label differs from the pass before.  The stop
 *                 is exact: equal labels reproduce the means bit for bit.  The reported means are update(final labels) in every case, so
 *                 iters = 0 gives the weighted means of the seeds' Voronoi cells.  dev_passes [A] int32 (may be NULL) = the p reached (iters
 *                 when the labels never stood still).
 *   7 outputs     dev_label [A, K] int32 (may be NULL); dev_count [A, n_modes] int32 = the members of mode i; dev_prob [A, n_modes] = W_i -- the
 *                 mass of the samples with label -1 is simply missing from the sum, the probabilities are NOT renormalised; dev_mean
 *                 [A, n_modes, T_pred, 2] (may be NULL), in Y's own coordinates (a mode that never had mass reports its seed row); dev_cov
 *                 [A, n_modes, T_pred, 3] (may be NULL) = (Cxx, Cyy, Cxy): with c_k = ((Y[r_k, t, 0] - mean_i[t, 0]) * unit_x, (Y[r_k, t, 1] -
 *                 mean_i[t, 1]) * unit_y) over the members of mode i in increasing k, Cxx = (sum w_k * (c_kx * c_kx)) / W_i + var_floor, Cyy
 *                 alike, Cxy = (sum w_k * (c_kx * c_ky)) / W_i; three zeros (no floor) for a mode with W_i == 0.  var_floor is in the caller's
 *                 units squared.
 *   8 likelihood  only with dev_fut: dev_out [A, n_h, 2] (then required) and dev_frame [A, T_pred] (may be NULL).  The counting rule, g, the
 *                 floor, the per-horizon mean and last-frame reduction and the zeros when nothing is counted are desire_kde_nll's steps 7 - 8.
 *                 For a counted (a, t) mode i is USABLE when prob_i > 0 and det > DESIRE_KDE_MIN_DET_RATIO * Cxx * Cyy, det = Cxx * Cyy - Cxy * Cxy.
 *                 d = ((mean_i[t, 0] - g_x) * unit_x, (mean_i[t, 1] - g_y) * unit_y); l_i = logf(prob_i) + (-0.5f * ((Cyy * (d_x * d_x) -
 *                 (2.f * Cxy) * (d_x * d_y)) + Cxx * (d_y * d_y))) / det - logf(2 pi) - 0.5f * logf(det), left to right; M = the maximum of the
 *                 l_i (fmaxf, from -inf); l = M + logf(sum of expf(l_i - M) over the usable modes in increasing i, from 0.f).  The frame's value is
 *                 l where l > log_floor, else log_floor (a NaN among them, and a frame without a usable mode).
 * A result depends on its agent's rows, order, scores and targets only -- not on the grid, the rest of the batch, DESIRE_FLAG_COMPACT_* or the
 * last desire_encode.  An absent slot's zero rows coincide: it reports count (K, 0, ...), zero spread plus var_floor, and needs no validity input.
 * One launch, stream-ordered, capturable, no host wait, no allocation, no scratch; bitwise reproducible.  host_horizons, n_h and log_floor are
 * read (and checked) only with dev_fut.
 * LDS plan: one workgroup stages all T_pred frames of all K samples of a chunk of slots next to the n_modes running means, the covariances and the
 * per-sample words; one agent must fit: 8 * (K + n_modes) * (T_pred | 1) + 12 * n_modes * T_pred + 8 * (T_pred | 1) + 12 * K + 8 * n_modes + 16
 * <= 61440 bytes -- e.g. (K 20, T_pred 40, n 6), (K 130, T_pred 9, n 4), (K 64, T_pred 9, n 16), (K 3, T_pred 200, n 3).  K beyond 64 is served
 * (a group's lanes loop), not refused.
 * DESIRE_ERR_ARG with a desire_last_error text, and nothing is launched or written: n_modes outside 1 .. min(K, DESIRE_MODES_MAX); t_end outside
 * 1 .. T_pred; iters outside 0 .. DESIRE_MODES_MAX_ITERS; a unit that is not finite and > 0; a var_floor that is negative or not finite; a NULL
 * dev_Yhat / dev_order / dev_count / dev_prob; dev_out or dev_frame without dev_fut; dev_fut without dev_out or host_horizons; with dev_fut bad
 * horizons or a non-finite log_floor; a NULL handle; a ref_compat handle; a (K, T_pred, n_modes) beyond the LDS plan. */
#define DESIRE_MODES_MAX 16
#define DESIRE_MODES_MAX_ITERS 32
int desire_fit_modes(desire_handle* h, const float* dev_Yhat, const int32_t* dev_order, const float* dev_score, const float* dev_fut,
                     int32_t n_modes, int32_t t_end, int32_t iters, float unit_x, float unit_y, float var_floor,
                     const int32_t* host_horizons, int32_t n_h, float log_floor,
                     int32_t* dev_label, int32_t* dev_count, float* dev_prob, float* dev_mean, float* dev_cov, int32_t* dev_passes,
                     float* dev_out, float* dev_frame, void* stream);

/* ---- n scene modes with covariances per window: what joint consumers take -- n scene modes, one probability per mode for the window and, for
 * every agent of that mode, a mean trajectory and a 2 x 2 covariance per frame, consistent across the agents -- fitted to the window's K weighted
 * WORLDS (world k = sample k of every slot together) by desire_fit_modes' weighted Lloyd iteration with `sample of an agent` read as `world of a
 * window`, and the joint likelihood of the ground truth under exactly that mixture: log sum_modes p_m prod_agents N(g | mean, cov).  Layouts are
 * desire_select_worlds': agent a = scene * mno + slot, row r_k = (scene * K + k) * mno + slot.  All arithmetic is fp32, every operation rounded
 * once (no fused multiply-add), every sum runs in one fixed sequence (over k, t or the slots in increasing index from 0.f); no float atomics.
 *   1 taking part dev_present [A] uint8 (may be NULL: every slot takes part).  Slot s takes part iff dev_present[a] != 0.  The rows of a slot that
 *                 does not take part are never read (under DESIRE_FLAG_COMPACT_* they may hold anything).
 *   2 weights     W_k = desire_select_worlds' step 6 on dev_wscore [n_scenes, K]: m = max_k s_k, e_k = expf(s_k - m), W_k = e_k / sum_k e_k in
 *                 increasing k from 0.f; 1.f / K when dev_wscore is NULL or any score of the window is not finite.
 *   3 seeds       c_i = dev_worder[scene, i] for i < n_modes (desire_joint_metrics' dev_jorder, or desire_select_worlds' dev_worder, which puts
 *                 mutually distinct worlds first); mean_i[s, t] = Y[r_{c_i}, t, :] for every taking-part slot s and t < T_pred.  Only these
 *                 n_modes entries of the row are read, through desire_fit_modes' check: the window is BAD when one of them lies outside 0 .. K-1 or
 *                 repeats an earlier one.  A BAD window gets labels -1, counts 0, prob, mean and cov 0.f, passes 0 and log_floor at every counted
 *                 frame.  No case reads outside dev_Yhat.
 *   4 distance    d_s(k, i) = desire_fit_modes' step 3 on slot s: the sum over t < t_end, from 0.f in increasing t, of (a * a + b * b), a =
 *                 (Y[r_k, t, 0] - mean_i[s, t, 0]) * unit_x, b = (Y[r_k, t, 1] - mean_i[s, t, 1]) * unit_y.  D(k, i) = the sum of d_s(k, i) over
 *                 the taking-part slots, in increasing slot from 0.f.
 *   5 assign      desire_fit_modes' step 4 on D(k, i): walking i = 0 .. n_modes-1, strict <, ties to the lower i, a NaN is never chosen; every
 *                 D(k, i) a NaN: label_k = -1, and world k is left out of everything below.
 *   6 update      W_i = the sum of W_k over the worlds with label_k = i, in increasing k from 0.f.  When W_i > 0: mean_i[s, t, c] = (the sum of
 *                 W_k * Y[r_k, t, c] over the same worlds in the same order) / W_i for every taking-part slot s and every t < T_pred.  A mode
 *                 without members, or with W_i == 0, keeps the means it has.
 *   7 iteration   desire_fit_modes' step 6: labels = assign(seed means); for p = 1 .. iters: update, assign, stop when no label differs from the
 *                 pass before.  The stop is exact; the reported means are update(final labels) in every case.  dev_passes [n_scenes] int32 (may
 *                 be NULL) = the p reached.  There is no special case: a window with nobody taking part runs the same sequence (every D is 0.f,
 *                 every world gets label 0, the fit stops at p = 1); a world with a NaN among the frames t < t_end of a taking-part row gets label
 *                 -1, and as a seed it is a mode nobody joins.
 *   8 outputs     dev_label [n_scenes, K] int32 (may be NULL); dev_count, dev_prob [n_scenes, n_modes] (required) = the members and W_i of mode
 *                 i, NOT renormalised; dev_mean [n_scenes, n_modes, mno, T_pred, 2] (may be NULL), in Y's own coordinates (a mode that never had
 *                 mass reports its seed's rows); dev_cov [n_scenes, n_modes, mno, T_pred, 3] (may be NULL) = (Cxx, Cyy, Cxy) by desire_fit_modes'
 *                 formula per slot over the mode's member worlds in increasing k, with W_k and W_i: three zeros (no floor) for a mode with
 *                 W_i == 0.  The slots that do not take part get zeros in dev_mean and dev_cov.
 *   9 likelihood  only with dev_fut [n_scenes, T_pred, mno, 3]: dev_out [n_scenes, n_h, 2] (then required) and dev_frame [n_scenes, T_pred] (may
 *                 be NULL).  c(a, t) and g are desire_kde_nll's.  C_t = the taking-part slots counted at t, c_t their number; frame t counts iff
 *                 c_t >= 1.  Mode i is USABLE at t when prob_i > 0 and every slot of C_t has det_s > DESIRE_KDE_MIN_DET_RATIO * Cxx * Cyy, det_s =
 *                 Cxx * Cyy - Cxy * Cxy.  L_i starts as logf(prob_i); for every slot of C_t in increasing slot, L_i = ((L_i + quad_s / det_s) -
 *                 logf(2 pi)) - 0.5f * logf(det_s), left to right, with d = ((mean_i[s, t, 0] - g_x) * unit_x, (mean_i[s, t, 1] - g_y) * unit_y) and
 *                 quad_s = -0.5f * ((Cyy * (d_x * d_x) - (2.f * Cxy) * (d_x * d_y)) + Cxx * (d_y * d_y)): desire_fit_modes' expressions.  M = the
 *                 maximum of the L_i (fmaxf, from -inf); l = M + logf(sum of expf(L_i - M) over the usable modes in increasing i, from 0.f).  The
 *                 frame's value is v = l / (float)c_t -- nats per agent, comparable with the per-agent calls -- where v > log_floor, else
 *                 log_floor (a NaN among them, and a frame without a usable mode); 0.f for a frame that does not count.  The per-horizon mean and
 *                 last-frame reduction and the zeros when nothing is counted are desire_kde_nll's steps 7 - 8 with `agent` read as `window`.
 * ANCHOR: at mno = 1 with the slot present, every output has the bits of desire_fit_modes given the same order row, dev_wscore holding that
 * agent's scores and the same dev_fut (0.f + x is exact, x / 1.f is exact).
 * A window's result depends on that window's taking-part rows, order row, scores and targets only -- not on the grid, the batch, the chunks the
 * slots are cut into, DESIRE_FLAG_COMPACT_* or the last desire_encode.  One launch, stream-ordered, capturable, no host wait, no allocation, no
 * scratch; bitwise reproducible.  host_horizons, n_h and log_floor are read (and checked) only with dev_fut.
 * LDS plan: one workgroup owns one window and walks its taking-part slots in chunks, once per pass: per chunk all T_pred frames of the K worlds'
 * rows next to the n_modes means, the chunk's distances and the likelihood's terms; what crosses a chunk border is the sum of d_s and the chain
 * of L_i, both in increasing slot: the bits of an unchunked walk.  One slot must fit next to the per-window words: 8 * (K + n_modes) * (T_pred | 1)
 * + 20 * n_modes * T_pred + 12 * K * n_modes + 12 * K + 20 * n_modes + 4 * n_modes * ceil(K / 32) + 12 * T_pred + 4 * mno <= 61440 bytes -- e.g.
 * (mno 256, K 20, T_pred 40, n 6): 4 slots per chunk; (K 70, T_pred 6, n 4), (K 3, T_pred 200, n 3).
 * DESIRE_ERR_ARG with a desire_last_error text, and nothing is launched or written: n_modes outside 1 .. min(K, DESIRE_MODES_MAX); t_end outside
 * 1 .. T_pred; iters outside 0 .. DESIRE_MODES_MAX_ITERS; a unit that is not finite and > 0; a var_floor that is negative or not finite; a NULL
 * dev_Yhat / dev_worder / dev_count / dev_prob; dev_out or dev_frame without dev_fut; dev_fut without dev_out or host_horizons; with dev_fut bad
 * horizons or a non-finite log_floor; a NULL handle; a ref_compat handle; a (K, mno, T_pred, n_modes) beyond the LDS plan. */
int desire_fit_scene_modes(desire_handle* h, const float* dev_Yhat, const uint8_t* dev_present, const int32_t* dev_worder,
                           const float* dev_wscore, const float* dev_fut,
                           int32_t n_modes, int32_t t_end, int32_t iters, float unit_x, float unit_y, float var_floor,
                           const int32_t* host_horizons, int32_t n_h, float log_floor,
                           int32_t* dev_label, int32_t* dev_count, float* dev_prob, float* dev_mean, float* dev_cov,
                           int32_t* dev_passes, float* dev_out, float* dev_frame, void* stream);

/* ---- predicted occupancy maps: how likely is it that somebody stands in this cell of the frame at horizon h, or at any time before it.  The K
 * samples of every agent, weighted, are rasterised onto an Oh x Ow grid over the normalised frame [0, 1) x [0, 1).  Layouts are the evaluation
 * calls': agent a = scene * mno + slot, row r_k = (scene * K + k) * mno + slot, dev_fut [n_scenes, T_pred, mno, 3], host_horizons as in
 * desire_ranked_errors (strictly increasing, 1 .. T_pred, n_h <= 8, read at call time, by value).  All arithmetic is fp32, every operation is
 * rounded once (no fused multiply-add); no float atomics.
 *   1 counted     exactly one of dev_fut and dev_present is non-NULL, as in desire_joint_metrics.  With dev_fut: c(a, t) =
 *                 dev_fut[scene, t, slot, 0] != 0 (evaluation).  With dev_present [A] uint8: c(a, t) = dev_present[a] != 0 for every t (prediction).
 *   2 weights     w_k of agent a is desire_kde_nll's step 1 exactly: NULL dev_score: 1.f / K; else m = max_j s_j, e_k = expf(s_k - m), w_k =
 *                 e_k / sum_j e_j, once per agent; 1.f / K for an agent with a non-finite score.  The same kernel fills the same scratch, so the
 *                 two calls are ordered by the stream like any two calls on one handle.
 *   3 cell        for a position (x, y): fx = floorf(x * (float)Ow), fy = floorf(y * (float)Oh), one rounded multiply each.  The position is IN
 *                 FRAME iff 0 <= fx <= Ow - 1 and 0 <= fy <= Oh - 1; every other position is OFF FRAME: a NaN, x = 1.0 exactly, negatives.  There
 *                 is no clamp (unlike the scene lookup: mass must not pile up on the border).  cell = (int)fy * Ow + (int)fx.
 *   4 visits      sample k of agent a VISITS cell c for horizon h -- DESIRE_OCC_AT: frame h - 1 is counted, its position is in frame and its
 *                 cell is c.  DESIRE_OCC_UNTIL: some counted frame t < h has an in-frame position in cell c.  Either way a sample contributes
 *                 to a cell at most once, however often it returns to it.
 *   5 marginal    p_a(h, c) = sum_k w_k * [k visits c], in increasing k from 0.f.
 *   6 window maps the agents are walked in increasing slot.  dev_exp [n_scenes, n_h, Oh, Ow] (may be NULL) = E, the sum of p_a from 0.f: the expected
 *                 number of agents.  dev_occ [n_scenes, n_h, Oh, Ow] (required) = 1.f - q, q starting at 1.f and q = q * (1.f - p_a) per agent: the
 *                 probability that at least one agent is there, agents being independent given the window.  An agent with p_a(h, c) = 0 leaves
 *                 both unchanged (adding 0.f and multiplying by 1.f are exact).
 *   7 columns     per agent, each [A, n_h], each may be NULL, each a sum over k in increasing k from 0.f; zeros for an agent with no counted frame.
 *                 dev_off  = the weight of the samples that are off frame -- AT: at frame h - 1, when it is counted; UNTIL: at any counted t < h.
 *                 dev_viol = the weight of the samples that visit a cell whose byte of the window's mask is 0 ("not traversable").  Needs
 *                            dev_mask [n_masks, Oh, Ow] uint8 and dev_mask_of_scene [n_scenes] int32 on the device (entries < n_masks: the
 *                            caller's promise); a scene whose entry is negative gets zeros.
 *                 dev_hit  = p_a(h, cell of g(a, h - 1)), g = (fut_x * sx, fut_y * sy) rounded once, the scaled target of desire_ranked_errors:
 *                            the mass on the ground truth's cell.  With dev_fut and DESIRE_OCC_AT only; 0 when frame h - 1 is not counted or g is
 *                            off frame.
 *   8 A window's results depend on that window's rows, scores and targets only -- not on the grid of workgroups, the batch or
 *     DESIRE_FLAG_COMPACT_*.  Bitwise reproducible, stream-ordered, capturable, no host wait, no allocation (the weights' scratch is desire_create's).
 * LDS plan: one workgroup owns one (window, horizon, band of grid rows): three floats per cell of the band (E, q, one agent's marginal), in
 * UNTIL a fourth word (the last sample that reached the cell), next to 20 bytes per position of a chunk of at most 512 positions of one agent,
 * 61440 bytes in all.  A grid beyond that -- 4266 cells in AT, 3200 in UNTIL at a full chunk -- is cut into bands of whole rows, each band a
 * workgroup that reads the window's rows again; a cell's sequence of operations is the same in every cut.  Every Oh, Ow <= 1024 and every
 * (mno, K, T_pred) of a handle is served.
 * DESIRE_ERR_ARG with a desire_last_error text, and nothing launched or written: a NULL handle / dev_Yhat / dev_occ / host_horizons; bad
 * horizons; a mode other than the two; Oh or Ow outside 1 .. 1024; both or neither of dev_fut / dev_present; dev_hit without dev_fut or in
 * UNTIL; dev_viol without both mask arguments; a ref_compat handle. */
#define DESIRE_OCC_AT 0       /* the frame h - 1 */
#define DESIRE_OCC_UNTIL 1    /* swept: any counted frame t < h */
#define DESIRE_OCC_MAX_SIDE 1024
int desire_occupancy(desire_handle* h, const float* dev_Yhat, const float* dev_fut, const uint8_t* dev_present,
                     const float* dev_score, const int32_t* host_horizons, int32_t n_h, int32_t mode,
                     int32_t Oh, int32_t Ow, const uint8_t* dev_mask, const int32_t* dev_mask_of_scene,
                     float* dev_occ, float* dev_exp, float* dev_hit, float* dev_viol, float* dev_off, void* stream);

/* ---- hipGraph capture: desire_graph_begin(h, stream); any stream-ordered desire_* calls on that stream (desire_forward,
 * desire_backward, desire_clip_grads, desire_ioc_step ...) ; desire_graph_end -> graph id; desire_graph_launch replays them with
 * the SAME device pointers.  For launch-bound shapes (small batches, the training step, the agent-sharded IOC loop).  Calls
 * that synchronise or read back to the host, and desire_adam_step (per-call step size), cannot be captured.  `stream` must be an
 * explicit non-default stream. */
int desire_graph_begin(desire_handle* h, void* stream);
int desire_graph_end(desire_handle* h, void* stream, int32_t* graph_id);
int desire_graph_launch(desire_handle* h, int32_t graph_id, void* stream);

/* ---- agent-sharded IOC (BASELINE north_star / SURVEY.md 8(e) E1: "agents shard across the GPUs with an RCCL all-gather
 * only for the social-pooling neighbour exchange").  The handle of rank g is created with mno = the slots it owns
 * (m_loc); every scene then has nranks * m_loc agents.  Everything before the IOC is per-agent and runs unchanged
 * (desire_encode / desire_sample); one IOC time step is one desire_ioc_step call, and the CALLER all-gathers the hidden
 * states in between (desire_amd/dist.py: ShardedIoc does it with torch.distributed = RCCL).  Gathered layouts, rank-major:
 *   Yall      [nranks][n_scenes*K][m_loc][T_pred][2]   decoded positions of every rank   (gathered once per pass)
 *   plast_all [nranks][n_scenes][m_loc][2]             last observed positions           (gathered once)
 *   valid_all [nranks][n_scenes][m_loc]                presence flags, uint8              (gathered once)
 *   Hall      [nranks][n_scenes*K*m_loc][H]            h_{t-1} of every rank              (gathered before every step)
 * dev_h_state [R_loc, H] (in: h_{t-1} of the local rows, out: h_t) and dev_score_state [R_loc] are the caller-held
 * recurrent state; desire_ioc_finish applies the regression head (Y += dY) and writes the scores.
 * desire_device_buffer exposes the handle's workspace tensors ("HxHy" [A,2H], "p_last" [A,2], "valid" [A] uint8,
 * "Y0" [R,T,2]) so they can be gathered without a host round trip. */
int desire_device_buffer(desire_handle* h, const char* name, void** dev_ptr, size_t* bytes);
int desire_ioc_step(desire_handle* h, int32_t t, int32_t rank, int32_t nranks, const float* dev_Yall,
                    const float* dev_plast_all, const uint8_t* dev_valid_all, const float* dev_Hall,
                    float* dev_h_state, float* dev_score_state, void* stream);
int desire_ioc_finish(desire_handle* h, const float* dev_h_state, const float* dev_score_state, float* dev_Y,
                      float* dev_score, void* stream);
/* The same agent-sharded pass WITHOUT a collective and without the host in the step loop: every rank owns an exchange region (its
 * blocks of the four gathered arrays above, two parities of hidden states, one progress counter), exported as a 64-byte
 * hipIpcMemHandle by desire_peer_export and mapped by the other ranks with desire_peer_open(h, rank, nranks, peer, handle) -- over xGMI
 * when the peer is another GPU, the same HBM when two ranks share a device.  How the handles travel is the caller's business
 * (desire_amd/dist.py: PeerShardedIoc uses torch.distributed.all_gather_object once); open the own rank with a NULL handle.  After
 * every rank has opened every peer (barrier), desire_ioc_peer_pass(h, dev_Y inout [R_loc, T_pred, 2], dev_score out [R_loc], stream)
 * enqueues the whole refinement -- publish, then per step: one-wave wait on the peers' counters, the step kernel reading their hidden
 * states IN PLACE, counter bump -- dims.iters times, with nothing but kernel launches (capturable by desire_graph_*).  A peer that
 * never arrives makes the bounded wait give up (a few seconds); the NEXT call then fails with DESIRE_ERR_HIP.  Results are bit-identical to
 * the desire_ioc_step loop.  desire_peer_close unmaps / frees (desire_destroy calls it). */
int desire_peer_export(desire_handle* h, uint8_t* handle_out64, size_t* bytes_out);
int desire_peer_open(desire_handle* h, int32_t rank, int32_t nranks, int32_t peer, const uint8_t* handle64);
int desire_ioc_peer_pass(desire_handle* h, float* dev_Y, float* dev_score, void* stream);
int desire_peer_close(desire_handle* h);
/* Whether a bounded wait of the passes enqueued so far has given up (*timed_out = 1): meaningful once the caller has synchronised the stream
 * the pass ran on -- a pass is stream-ordered, so this is the earliest point at which ITS outcome is known; without the query a caller only
 * learns of a timed-out pass from the next desire_ioc_peer_pass.  Does not clear the condition. */
int desire_peer_status(desire_handle* h, int32_t* timed_out);
/* Ranks inside ONE process (one process driving several devices with peer access enabled) attach each other's regions by device
 * pointer: desire_peer_region gives a handle's own region, desire_peer_open_ptr takes the peer's (hipIpc handles cannot be opened by
 * the process that exported them).  Every rank's pass must then run on a HARDWARE queue of its own: a pass parks a one-wave wait
 * kernel on its stream until the peers catch up, and two streams that the runtime multiplexes onto one queue (it maps a process's
 * streams of ONE device onto 4 queues) would wait for each other until the time-out.  Streams of different devices never share a
 * queue; several ranks on one device belong in separate processes (tests/test_gpu_peer_ioc.py). */
int desire_peer_region(desire_handle* h, void** dev_region, size_t* bytes);
int desire_peer_open_ptr(desire_handle* h, int32_t rank, int32_t nranks, int32_t peer, void* dev_region);

/* ---- training (the reference builds tf.gradients(cost) + Adam and never runs them: model/model.py:388-403) ----
 * desire_set_training(h,1) allocates the activation-save and gradient buffers; a desire_forward made afterwards keeps
 * what backward needs.  desire_backward computes d(loss)/d(weight) for the loss of DESIGN.md section 8 into ONE flat
 * fp32 device buffer (natural TF layouts; desire_grad_buffer exposes it so a multi-GPU caller can all-reduce it).
 * Frozen batch-norm parameters are constants (no gradient).  desire_set_training(h,0) hands the trained master weights back to
 * the handle (desire_get_weight returns them, inference keeps using the device operands the last desire_adam_step rebuilt);
 * enabling training again starts from them with the Adam moments at zero (desire_adam_state to carry moments across). */
int desire_set_training(desire_handle* h, int enable);
/* The reference's OWN loss for its 5-wide output layer (model/model.py:315-366: output_w / output_b on the recurrent state, get_coef
 * :552-565, -log max(N(next position | mux, muy, sx, sy, rho), 1e-20) :494-550, id == 0 masking :351-366, mean :374-376) as an extra
 * term of the training loss: weight x mean over the counted (object, observed frame) pairs, teacher-forced over the X encoder's
 * observed steps (target of frame t = the position in frame t + 1; frame T_obs is the first future frame).  desire_backward then
 * also fills the gradients of "gauss_head/w|b" -- the head desire_rollout / sample() read, which no other term reaches -- and adds
 * the term's gradient to the X encoder's, step by step.  weight = 0 (default) switches the term off. */
int desire_set_head_loss(desire_handle* h, float weight);
/* ---- best-of-many / soft-min reconstruction term.  The sample-generation loss of the paper averages the K samples' errors, which pulls every
 * sample toward the one observed future; letting the best sample (Bhattacharyya et al. 2018's best-of-many objective, Social-GAN's variety loss)
 * or a soft-min over the samples carry the reconstruction gradient keeps the K samples apart.  Layouts, the counting rule and g are
 * desire_ranked_errors': agent a = scene * mno + slot, row r_k = (scene * K + k) * mno + slot, dev_fut [n_scenes, T_pred, mno, 3], g_t =
 * (fut_x * sx, fut_y * sy) rounded once; frame t COUNTS when dev_fut[scene, t, slot, 0] != 0; nfut[a] = the number of counted frames and lmask[a] =
 * present at the last observed frame (the handle's "valid", left by the last desire_encode / desire_forward) && nfut[a] > 0, as in desire_losses.
 * All arithmetic is fp32, every operation rounded once (no fused multiply-add); expf / logf are the device library's.
 *   1 error       e[a, k] = (sum over the counted t, in increasing t from 0.f, of sqrtf(dx * dx + dy * dy)) / nfut[a], dx = Y[r_k, t, 0] - g_t.x,
 *                 dy = Y[r_k, t, 1] - g_t.y; e[a, k] = 0 where lmask[a] = 0.
 *   2 winner      a walk in increasing k: winner = 0, m = e[a, 0]; k replaces it when e[a, k] < m (strict: ties stay with the lower k) or when m
 *                 is a NaN and e[a, k] is not (a NaN never wins against a number).  The walk is the same in every mode.
 *   3 weights     DESIRE_RECON_MEAN:    w[a, k] = 1.f / K;                 recon[a] = (sum of e[a, k] in increasing k from 0.f) / K.
 *                 DESIRE_RECON_MIN:     w[a, k] = k == winner ? 1.f : 0.f; recon[a] = m.
 *                 DESIRE_RECON_SOFTMIN: x_k = expf(-(e[a, k] - m) / tau); S = the sum of x_k in increasing k from 0.f; w[a, k] = x_k / S;
 *                                       recon[a] = m - tau * logf(S / K).  tau is in normalised units; tau -> inf is MEAN, tau -> 0 is MIN, and
 *                                       d recon / d e_k = w_k exactly, so w is a constant of the backward pass.
 * desire_recon_weights is the stand-alone op: dev_e [A, K], dev_w [A, K], dev_winner [A] int32, dev_recon [A]; each may be NULL (it then goes to
 * the workspace tensor "recon_e" / "recon_w" / "recon_win" / "recon_val"), and what is written does not depend on which are.  It needs no training
 * mode.  Stream-ordered, no host wait, no atomics, no scratch: bitwise reproducible; the first call allocates the four workspace tensors, later
 * calls are capturable.  A result depends on its agent's rows and targets only -- not on the grid, the batch or DESIRE_FLAG_COMPACT_*.  K has no
 * limit; one row of T_pred positions with its targets must fit the kernel's LDS (T_pred <= 7680).  DESIRE_ERR_ARG, and nothing is launched: a NULL
 * handle / dev_fut / dev_Yhat, a mode outside 0 .. 2, in mode SOFTMIN a tau that is not finite or <= 0, a ref_compat handle, T_pred too long.
 * desire_set_recon_loss chooses the term of the TRAINING loss (default DESIRE_RECON_MEAN, which leaves the launch sequence and every bit of
 * every output as they were; tau is ignored there and in MIN).  In MIN and SOFTMIN desire_backward runs step 1 - 3 on the full layout (before the
 * gather of DESIRE_FLAG_COMPACT_ROWS) and takes
 *   d loss / d Y0[r_k, t] = (lmask[a] && counted(t) && nrm > 0) ? w[a, k] / (nvalid * nfut[a] * nrm) * (Y0[r_k, t] - g_t) : 0,  nrm = ||Y0[r_k, t] - g_t||,
 * and slot 0 (recon) of desire_train_loss / desire_train_loss_async is the mean of recon[a] over the counted agents.  Nothing else changes: KL,
 * the IOC cross-entropy (its target still uses the detached Y0) and the IOC regression term keep their mean over K.  The mode can be changed
 * between steps (not inside a captured graph: it is a host value, baked into the capture). */
#define DESIRE_RECON_MEAN 0
#define DESIRE_RECON_MIN 1
#define DESIRE_RECON_SOFTMIN 2
int desire_set_recon_loss(desire_handle* h, int32_t mode, float tau);
int desire_recon_weights(desire_handle* h, const float* dev_fut, const float* dev_Yhat, int32_t mode, float tau,
                         float* dev_e, float* dev_w, int32_t* dev_winner, float* dev_recon, void* stream);
/* ---- the scope of that term: per agent (above), or per window over its K joint futures.  Sample k of every agent of a window is one joint
 * future, a "world" (desire_joint_metrics, desire_select_worlds, desire_fit_scene_modes, desire_plan_risk*).  Per agent, every agent picks its own
 * best k and no single world is pulled toward the observed scene; in scope SCENE the best WORLD of a window -- or a soft-min over its worlds --
 * carries the reconstruction gradient of every agent of the window (the scene-level variety loss).  Layouts, lmask, nfut, g and the fp32 rule
 * (every operation rounded once, no fused multiply-add, the device library's expf / logf) are desire_recon_weights'; window(a) = a / mno; a sum
 * "in increasing X" starts from 0.f.
 *   1 error       e[a, k]: step 1 of desire_recon_weights, the same bits on the same inputs.
 *   2 world error count[w] = the number of slots of window w with lmask = 1 (int32).  E[w, k] = (the sum over the slots with lmask = 1, in
 *                 increasing slot, of e[a, k]) / (float)count[w]; E[w, k] = 0.f where count[w] = 0.
 *   3 winner      winner[w]: the walk of step 2 of desire_recon_weights on E[w, .] (strict, ties to the lower k, a NaN never beats a number).
 *   4 weights     DESIRE_RECON_MEAN:    W[w, k] = 1.f / K;                  R[w] = (the sum of E[w, k] in increasing k) / K.
 *                 DESIRE_RECON_MIN:     W[w, k] = k == winner ? 1.f : 0.f;  R[w] = E[w, winner].
 *                 DESIRE_RECON_SOFTMIN: x_k = expf(-(E[w, k] - m) / tau), m = E[w, winner]; S = the sum of x_k in increasing k; W[w, k] = x_k / S;
 *                                       R[w] = m - tau * logf(S / K).
 * desire_recon_weights_scene is the stand-alone op: dev_e [A, K], dev_E [n_scenes, K], dev_count [n_scenes] int32; dev_w [A, K] with w[a, k] =
 * W[window(a), k] on EVERY slot of the window (the gradient masks the slots that do not count itself), dev_winner [A] int32 = winner[window(a)]
 * and dev_recon [A] = R[window(a)], on every slot too.  Each may be NULL (it then goes to the workspace tensor "recon_e" / "recon_E" /
 * "recon_cnt" / "recon_w" / "recon_win" / "recon_val"), and what is written does not depend on which are.  It needs no training mode.  Two
 * launches (the streaming pass of desire_recon_weights without its per-agent walk, then one workgroup per window), stream-ordered, no host wait,
 * no atomics, no scratch: bitwise reproducible; the first call allocates the workspace tensors, later calls are capturable.  K has no limit;
 * T_pred as for desire_recon_weights.  At mno = 1 w, winner and recon have the bits of desire_recon_weights.  DESIRE_ERR_ARG, and nothing is
 * launched: a NULL handle / dev_fut / dev_Yhat, a mode outside 0 .. 2, in mode SOFTMIN a tau that is not finite or <= 0, a ref_compat handle,
 * T_pred too long.
 * desire_set_recon_scope chooses the scope of the TRAINING loss's term (default DESIRE_RECON_SCOPE_AGENT: everything above as it is).  In scope
 * SCENE with mode MIN or SOFTMIN desire_backward runs steps 1 - 4 on the full layout where it ran desire_recon_weights' steps, the gradient is
 * the formula above with this w, and slot 0 of desire_train_loss* is
 *   L_recon = (sum over w of count[w] * R[w]) / (sum over w of count[w]),
 * the mean of recon[a] over the counted agents; d L_recon / d e[a, k] = W[window(a), k] / nvalid for a counted agent.  In mode MEAN the scope is
 * ignored (the mean over k of a mean over agents is the mean over both): the default's launches and bits.  KL, the IOC cross-entropy and the IOC
 * regression term keep their mean over K.  SCENE allocates "recon_E" / "recon_cnt" (and the four above) when it is set, so that no step
 * allocates.  A host value like the mode: it can be changed between steps, not inside a captured graph.  DESIRE_ERR_ARG: a NULL handle, a scope
 * outside 0 .. 1, T_pred too long; DESIRE_ERR_STATE: SCENE on a ref_compat handle. */
#define DESIRE_RECON_SCOPE_AGENT 0      /* default: per agent, as above */
#define DESIRE_RECON_SCOPE_SCENE 1
int desire_set_recon_scope(desire_handle* h, int32_t scope);
int desire_recon_weights_scene(desire_handle* h, const float* dev_fut, const float* dev_Yhat, int32_t mode, float tau,
                               float* dev_e, float* dev_E, int32_t* dev_count, float* dev_w, int32_t* dev_winner, float* dev_recon, void* stream);
/* ---- collision penalty on the K joint futures.  Every term above pulls samples toward the one observed future or does not see the other agents'
 * samples at all; this one makes the worlds themselves collision-free: a squared hinge in the distance of every pair of counted agents of one
 * (window, k) and frame.  Layouts are desire_joint_metrics': agent a = scene * mno + slot, row r_k = (scene * K + k) * mno + slot, window(a) = a /
 * mno, dev_fut [n_scenes, T_pred, mno, 3]; lmask, nfut, nvalid (= max(the number of agents with lmask, 1) as a float) and the counted frames are
 * desire_recon_weights' (the loss mask of desire_losses).  All arithmetic is fp32, every operation rounded once (no fused multiply-add), sqrtf and
 * the divisions correctly rounded; no float atomics; a sum "in increasing X" starts from 0.f.
 *   1 counted     cc(a, t) = lmask[a] && dev_fut[scene, t, slot, 0] != 0.
 *   2 pair        for slots i != j of one (window, k) and a frame t with cc(i, t) && cc(j, t): a = (Y[r_i, t, 0] - Y[r_j, t, 0]) * unit_x; b =
 *                 (Y[r_i, t, 1] - Y[r_j, t, 1]) * unit_y; q = a * a + b * b; r2 = radius * radius -- desire_joint_metrics' step 2, symmetric in i, j
 *                 bit for bit.  The pair TOUCHES at t iff q < r2: strict, false for a NaN; radius 0: nothing touches.
 *   3 penalty     for a touching pair dist = sqrtf(q); u = 1.f - dist / radius; phi = u * u; else phi = 0.  C1 at the radius, 1 at full overlap.
 *   4 per agent   s(i, k, t) = the sum over j != i, in increasing j, of phi_ij(t) (a pair that does not touch adds nothing).  col[i, k] = (the sum
 *                 over the counted frames of i, in increasing t, of s(i, k, t)) / nfut[i]; col[i, k] = 0.f where lmask[i] = 0.
 *   5 count       touch[w, k] (int32) = the number of (unordered pair, frame) that touch: an integer path.
 *   6 term        m[a] = (the sum of col[a, k] in increasing k) / (float)K.  S_l, l = 0 .. 255, = the sum of m[a] over the agents a = l, l + 256, ..
 *                 in increasing a (col is 0.f where lmask = 0); the 256 sums meet in a binary tree, S_l = S_l + S_(l + st) for l < st, st = 128, 64,
 *                 .., 1; L_col = S_0 / nvalid.  The mean over K, then the mean over the counted agents: the default reconstruction term's reduction.
 *   7 gradient    of L_col at weight 1.  For a touching pair with dist > 0: c_ij = (inv[i] + inv[j]) * (u / (radius * dist)), inv[a] = 1.f /
 *                 nfut[a]; X(i, t) = the sum over j != i in increasing j of c_ij * a, Y(i, t) the same with b (a pair at dist == 0 adds nothing:
 *                 the rule nrm > 0 has in the reconstruction gradient).  scale = -2.f / (nvalid * (float)K).  G[r_i, t, 0] = (X * unit_x) * scale,
 *                 G[r_i, t, 1] = (Y * unit_y) * scale; G = 0.f for frames and agents that are not counted.  This is d L_col / d Y[r_i, t, c] =
 *                 the sum over j of (1 / nfut[i] + 1 / nfut[j]) / (nvalid * K) * d phi_ij / d Y[r_i, t, c].  Each (i, t) gathers its own sum.
 * desire_collision_loss is the stand-alone op: dev_col [A, K], dev_touch [n_scenes, K] int32, dev_dY [R, T_pred, 2] = G, dev_term [1] = L_col; each
 * may be NULL (it then goes to the workspace tensor "col_val" / "col_touch" / "col_grad" / "col_term"), and what is written does not depend on
 * which are.  It needs no training mode (lmask comes from the handle's "valid", left by the last desire_encode / desire_forward, as in
 * desire_recon_weights).  Stream-ordered, no host wait, no scratch: bitwise reproducible; the first call allocates the workspace tensors, later
 * calls are capturable.  A window's col, touch and -- up to the common factor 1 / nvalid -- gradient depend on that window's rows and targets only.
 * LDS plan: one workgroup owns one (window, k) and stages its positions as desire_joint_metrics does, next to the gradient and s of the staged
 * frames parked slot-major (20 bytes per slot and frame in all); when the unit does not fit (256 slots x 40 frames) it walks the frames in chunks
 * -- 11 at 256 slots -- carrying the per-slot sums across them, with the bits of an unchunked walk.  Every (mno, T_pred) of a handle is served.
 * DESIRE_ERR_ARG with a desire_last_error text, and nothing is launched or written: a NULL handle / dev_fut / dev_Yhat; a radius that is negative
 * or not finite; a unit that is not finite and > 0; a ref_compat handle.
 * desire_set_collision_loss configures the term of the TRAINING loss (default weight 0, which leaves the launch sequence and every bit of every
 * output as they were).  With weight > 0 desire_backward runs steps 1 - 7 on its own "Y0", on the full layout (after the reconstruction gradient,
 * before the gather of DESIRE_FLAG_COMPACT_ROWS), and sets dY0 = dY0 + weight * G (the product rounded, then the sum); the trained loss is the
 * one above plus weight * L_col.  The term keeps its mean over K whatever desire_set_recon_loss / desire_set_recon_scope say, as KL and the IOC
 * terms do: every world should be collision-free, not only the winner.  The backward leaves col, touch and L_col of that step in "col_val",
 * "col_touch" and "col_term" (desire_device_buffer); desire_train_loss / desire_train_loss_async keep their layouts and values.  weight > 0
 * allocates the workspace tensors when it is set, so that no step allocates.  A host value like the recon mode: it can be changed between steps,
 * not inside a captured graph.  DESIRE_ERR_ARG: a NULL handle, a weight that is negative or not finite, a bad radius or unit; DESIRE_ERR_STATE: a
 * ref_compat handle. */
int desire_set_collision_loss(desire_handle* h, float weight, float radius, float unit_x, float unit_y);
int desire_collision_loss(desire_handle* h, const float* dev_fut, const float* dev_Yhat, float radius, float unit_x, float unit_y,
                          float* dev_col, int32_t* dev_touch, float* dev_dY, float* dev_term, void* stream);
/* ---- off-road penalty on the K joint futures.  desire_occupancy reports `violation`, the sample mass on cells a traversability mask forbids; this
 * term pushes it down: the squared distance, read off the distance field of the mask, of every counted position to the nearest traversable cell.
 * All arithmetic is fp32, every operation rounded once (no fused multiply-add), sqrtf and the divisions correctly rounded; no float atomics; a sum
 * "in increasing X" starts from 0.f.
 * desire_mask_distance: the exact distance field of a binary mask.  dev_mask [n_masks, Mh, Mw] uint8 with desire_occupancy's meaning (byte 0 = not
 * traversable), dev_field [n_masks, Mh, Mw] fp32.  For the cell (y, x): q = the min over the traversable cells (y', x') of the same mask of a * a +
 * b * b with a = (float)(x - x') * cell_x and b = (float)(y - y') * cell_y (two rounded products, one rounded sum); field = sqrtf(q): the distance
 * from the cell's centre to the nearest traversable centre in the caller's unit, 0.f on a traversable cell.  A mask with NO traversable cell gives
 * 0.f everywhere: no constraint, not an infinite one.  A min does not depend on the order of its operands; the device takes it in two passes (per
 * column the nearest traversable row, then per cell the min over the columns: the rounded expression is monotone in |y - y'|), with the bits of
 * the statement.  Mh, Mw: 1 .. DESIRE_OCC_MAX_SIDE; n_masks: 1 .. DESIRE_OFFROAD_MAX_MASKS.  Stream-ordered and capturable: it waits for nothing
 * and allocates nothing (dev_field itself holds the first pass's integers until the second overwrites them).  Not on the step path: a field is
 * built once per set of scenes.  DESIRE_ERR_ARG with a desire_last_error text, nothing launched: a NULL handle / dev_mask / dev_field; n_masks, Mh
 * or Mw out of range; a cell size that is not finite and > 0; a ref_compat handle.
 * desire_set_offroad_field attaches fields to the handle as desire_set_scene_grids attaches grids: dev_field [n_fields, Mh, Mw] is referenced, not
 * copied (it must outlive its use); host_field_of_scene [n_scenes] maps each window to a field and is copied to device words the handle owns: every
 * entry must be < n_fields, a NEGATIVE entry means the window has no field (it costs, counts and pushes nothing).  It may be called between steps
 * with the same field and another mapping.  The map goes up as desire_set_scene_grids' does, by a synchronous hipMemcpy from the caller's pageable
 * array: the host waits for the device's earlier work on the null stream, so a caller that changes the mapping every step gives up running ahead
 * of the device, and on a non-blocking stream the caller orders the copy against a step that still reads the map; not inside a captured graph.  DESIRE_ERR_ARG: a NULL argument, n_fields or a side
 * out of range, an entry >= n_fields, a ref_compat handle.
 * The penalty.  Layouts, lmask, nfut, nvalid and the counted frames cc(a, t) are desire_collision_loss': agent a = scene * mno + slot, row r_k =
 * (scene * K + k) * mno + slot.  D = the field of the agent's window, fMw = (float)Mw, fMh = (float)Mh.  Per counted (a, k, t) with (x, y) = Y[r_k,
 * t, 0 .. 1] in the normalised frame:
 *   1 lookup      xm = x * fMw; u = xm - 0.5f; uc = min(max(u, 0.f), (float)(Mw - 1)); x0 = (int)floorf(uc); x1 = min(x0 + 1, Mw - 1); fx = uc -
 *                 floorf(uc); likewise ym, v, vc, y0, y1, fy with Mh: cell centres sit on integers, and the lookup is clamped to them.  If x or y
 *                 is a NaN the item costs nothing, pushes nothing and counts nothing.
 *   2 distance    D00 = D[y0, x0], D01 = D[y0, x1], D10 = D[y1, x0], D11 = D[y1, x1]; h0 = D01 - D00; h1 = D11 - D10; top = D00 + fx * h0; bot =
 *                 D10 + fx * h1; vd = bot - top; d = top + fy * vd.
 *   3 penalty     e = d / scale; phi = e * e (scale in the field's unit).  0 on the road; continuous with a continuous gradient across the road's
 *                 edge (d -> 0), so a sample that crosses it between two steps changes neither by a jump; off the road the slope jumps at cell
 *                 lines, as any bilinear lookup's does.
 *   4 per agent   off[a, k] = (the sum over the counted frames of a, in increasing t, of phi) / nfut[a]; 0.f where lmask[a] = 0 or the window
 *                 has no field.
 *   5 count       count[w, k] (int32) = the number of counted (slot, frame)s of window w whose cell by desire_occupancy's step 3 -- floorf(xm),
 *                 floorf(ym), no clamp -- is IN FRAME and has D > 0.f there: the rule dev_viol applies to the mask, read off the field.  An
 *                 integer path.
 *   6 term        L_off = desire_collision_loss' step 6 on off: the mean over K, the 256 strided sums in increasing a, the binary tree, / nvalid.
 *   7 gradient    of L_off at weight 1.  sx = (h0 + fy * (h1 - h0)) * fMw, and sx = 0.f unless 0.f <= u <= (float)(Mw - 1) (the clamped lookup
 *                 does not move with x); sy = vd * fMh, 0.f unless 0.f <= v <= (float)(Mh - 1).  m = (2.f * e) / scale; coef = (1.f / nfut[a]) /
 *                 (nvalid * (float)K).  G[r_k, t, 0] = (m * sx) * coef; G[r_k, t, 1] = (m * sy) * coef; G = 0.f for whatever is not counted.
 *                 Every (row, t) owns its element: nothing scatters.
 * desire_offroad_loss is the stand-alone op on the fields set by desire_set_offroad_field: dev_off [A, K], dev_count [n_scenes, K] int32, dev_dY [R,
 * T_pred, 2] = G, dev_term [1] = L_off; each may be NULL (it then goes to the workspace tensor "off_val" / "off_count" / "off_grad" / "off_term"),
 * and what is written does not depend on which are.  It needs no training mode (lmask comes from the handle's "valid", as in
 * desire_collision_loss).  Stream-ordered, no host wait, no scratch: bitwise reproducible; the first call allocates the workspace tensors, later
 * calls are capturable.  LDS plan: desire_collision_loss' (one workgroup per (window, k), frame chunks with the bits of an unchunked walk), with
 * the window's field behind it when it fits (64 x 64 cells next to 32 slots x 40 frames do); else the four taps are read from global memory: the
 * same bits.  DESIRE_ERR_ARG, nothing launched or written: a NULL handle / dev_fut / dev_Yhat; a scale that is not finite and > 0; a ref_compat
 * handle.  DESIRE_ERR_STATE: no field set.
 * desire_set_offroad_loss configures the term of the TRAINING loss (default weight 0, which leaves the launch sequence and every bit of every
 * output as they were; the scale is then not read).  With weight > 0 desire_backward runs steps 1 - 7 on its own "Y0", on the full layout, after
 * the collision term and before the gather of DESIRE_FLAG_COMPACT_ROWS, and sets dY0 = dY0 + weight * G (the product rounded, then the sum); the
 * trained loss is the one above plus weight * L_off.  The term keeps its mean over K whatever desire_set_recon_loss / desire_set_recon_scope say.
 * The backward leaves off, count and L_off of that step in "off_val", "off_count" and "off_term"; desire_train_loss / desire_train_loss_async keep
 * their layouts and values.  weight > 0 needs a field to be set (DESIRE_ERR_STATE otherwise) and allocates the workspace tensors when it is set,
 * so that no step allocates.  A host value: it can be changed between steps, not inside a captured graph.  DESIRE_ERR_ARG: a NULL handle, a weight
 * that is negative or not finite, with weight > 0 a scale that is not finite and > 0; DESIRE_ERR_STATE: a ref_compat handle, no field. */
#define DESIRE_OFFROAD_MAX_MASKS 65535
int desire_mask_distance(desire_handle* h, const uint8_t* dev_mask, int32_t n_masks, int32_t Mh, int32_t Mw, float cell_x, float cell_y,
                         float* dev_field, void* stream);
int desire_set_offroad_field(desire_handle* h, const float* dev_field, int32_t n_fields, int32_t Mh, int32_t Mw,
                             const int32_t* host_field_of_scene);
int desire_set_offroad_loss(desire_handle* h, float weight, float scale);
int desire_offroad_loss(desire_handle* h, const float* dev_fut, const float* dev_Yhat, float scale, float* dev_off, int32_t* dev_count,
                        float* dev_dY, float* dev_term, void* stream);
/* ---- the same three terms on the REFINED trajectories.  The model's output is Y = Y0 + the sum over the IOC passes of dY_p ("Y_ref" of a training
 * step); the four settings above act on the decoder's samples Y0, and the one term that trains the refinement, the IOC regression term, is the plain
 * mean over K of ||Y - g||.  desire_set_refined_loss(recon, collision_weight, offroad_weight) -- default (0, 0, 0): the step as it is, its launches
 * and every bit -- moves them onto Y.  The IOC trajectories stay detached from Y0: what is added here reaches ioc/ * and, through Hx, the encoders
 * (and the scene CNN when images are attached), nothing else.  d loss / d Y enters the IOC backward at one point, "dYr" on the full layout, before
 * the gather of the slot classes and shared by every refinement pass; the terms are applied there in this order:
 *   recon = 1             the regression term follows desire_set_recon_loss / desire_set_recon_scope as they stand AT THE STEP: the weights are
 *                         desire_recon_weights' (scope SCENE: desire_recon_weights_scene's) on the refined errors e1[a, k] -- the error of Y against
 *                         the future with the loss mask and the counted frames of slot 0 -- and the gradient is the weighted formula of
 *                         desire_set_recon_loss with Y for Y0.  Slot 3 (regression) of desire_train_loss* then reports the term that is trained, by
 *                         slot 0's rule: the mean over the counted agents of the min / soft-min of e1, in scope SCENE of the window's term.  In mode
 *                         MEAN the flag is accepted and changes neither launches nor bits.  Weights and winners stay in "rrecon_e" / "rrecon_w" /
 *                         "rrecon_win" / "rrecon_val" (scope SCENE: also "rrecon_E" / "rrecon_cnt").
 *   collision_weight > 0  dYr = dYr + collision_weight * G (the product rounded, then the sum), G = step 7 of desire_collision_loss on Y with the
 *                         radius and units the handle holds from desire_set_collision_loss, whose own weight may be 0: that is how the refinement
 *                         alone is penalised.  col, touch and L_col(Y) of the step: "rcol_val" / "rcol_touch" / "rcol_term".
 *   offroad_weight > 0    the same with desire_offroad_loss' G on the fields of desire_set_offroad_field and the scale of desire_set_offroad_loss
 *                         (its weight may be 0): "roff_val" / "roff_count" / "roff_term".
 * Both penalties keep their mean over K whatever the recon mode says, as their Y0 twins do.  The trained loss is
 *   L_sgm + mean_counted(ce + reg') + cw * L_col(Y0) + ow * L_off(Y0) + collision_weight * L_col(Y) + offroad_weight * L_off(Y)   [+ head term]
 * with reg' the plain mean, or with recon = 1 and a mode other than MEAN the min / soft-min term of e1.  The layouts of desire_train_loss* do not
 * change.  Under DESIRE_FLAG_COMPACT_* the padded rows of Y hold anything; the kernels read uncounted slots through the loss mask only.  Workspace
 * is allocated here, never in a step; with everything off nothing is allocated.  Host values: they can be changed between steps, not inside a
 * captured graph.  Refusals, in this order, each leaving the handle's settings as they were: DESIRE_ERR_ARG: a NULL handle; recon not 0 or 1; a
 * weight that is negative or not finite.  DESIRE_ERR_STATE: a ref_compat handle; collision_weight > 0 with no radius > 0 set; offroad_weight > 0
 * with no field set, or with a scale that is not finite and > 0.  (recon = 1 with T_pred too long for desire_recon_weights: DESIRE_ERR_ARG.) */
int desire_set_refined_loss(desire_handle* h, int32_t recon, float collision_weight, float offroad_weight);
/* (dev_eps == NULL after desire_set_rng: the eps of the forward's draw is regenerated, see "device generator") */
int desire_backward(desire_handle* h, const float* dev_past, const float* dev_fut, const float* dev_eps, void* stream);
int desire_get_grad(desire_handle* h, const char* name, float* host_out, size_t n, void* stream);
int desire_grad_buffer(desire_handle* h, float** dev_ptr, size_t* n);
/* Loss terms of the last training-mode forward, means over present agents:
 * host_out5 = {recon, kld, cross_entropy, regression, n_present};  loss = sum of the first four. */
int desire_train_loss(desire_handle* h, const float* dev_fut, float* host_out5, void* stream);
/* The same values written to a DEVICE buffer dev_out8 [8] = {recon, kld, cross_entropy, regression, n_present, nll_head, grad_norm,
 * n_head}, stream-ordered and without synchronising: a training loop that reads the loss one step late (desire_amd/train.py) never
 * stalls the host behind the step it has just enqueued.  nll_head / n_head: the weighted Gaussian-head term of the last
 * desire_backward and the (object, frame) pairs it averaged over (0 while that loss is off); grad_norm: the pre-clip global norm of
 * the last desire_clip_grads. */
int desire_train_loss_async(desire_handle* h, const float* dev_fut, float* dev_out8, void* stream);
/* tf.clip_by_global_norm (model/model.py:390) on the flat gradient buffer, in place; host_norm_out (optional, may be
 * NULL: then no synchronisation) receives the pre-clip norm. */
int desire_clip_grads(desire_handle* h, float max_norm, float* host_norm_out, void* stream);
/* One tf.train.AdamOptimizer update (model/model.py:394; lr_t = lr*sqrt(1-b2^t)/(1-b1^t)) of the device master weights
 * from the flat gradient buffer, followed by a device-side rebuild of every packed operand.  No host round trip. */
int desire_adam_step(desire_handle* h, float lr, float beta1, float beta2, float eps, void* stream);
/* Optimiser state for checkpoints (the reference's Saver stores every global variable, Adam slots included, train.py:114): the
 * moments are the workspace tensors "Mflat" / "Vflat" (desire_device_buffer; the gradient buffer's flat layout), the step
 * counter of the bias correction is read (set = 0) or written (set = 1) through *step. */
int desire_adam_state(desire_handle* h, int32_t* step, int set);
/* Current value of a weight (the trained one in training mode), natural TF layout. */
int desire_get_weight(desire_handle* h, const char* name, float* host_out, size_t n, void* stream);

/* Per-kernel GPU time measured with hipEvents on the launch stream (enabled by
 * desire_set_profiling(h,1); adds two event records per kernel, nothing else).  Entries accumulate
 * over calls; desire_get_profile synchronises on them, copies up to *count (in: capacity) entries
 * to host_ms[i] / host_names[i], sets *count, and clears the list.  With host_ms == host_names ==
 * NULL it only reports the pending entry count. */
int desire_set_profiling(desire_handle* h, int enable);
int desire_get_profile(desire_handle* h, float* host_ms, const char** host_names, int32_t* count);

#ifdef __cplusplus
}
#endif
#endif /* DESIRE_HIP_H */
