// ctx.h -- the handle behind desire_handle* and the small host helpers shared by api.hip (inference ABI),
// train.hip and backward.hip (training ABI).  Host code only.
#pragma once
#include "../../include/desire_hip.h"
#include "gen_plan.h"
#include "ioc_plan.h"
#include "kernels.h"
#include "pack.h"
#include "workspace.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

int desire_fail(int code, const std::string& msg);            // sets the thread-local last-error text
#define fail desire_fail
#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess)                                                                       \
            return fail(DESIRE_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));            \
    } while (0)

inline int dev_malloc(void** p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess ? 0 : -1; }      // the allocator of workspace.h
inline void dev_free(void* p) { (void)hipFree(p); }

struct Prof { std::string name; hipEvent_t e0, e1; };

struct WSlot { size_t off; size_t n; };                       // a named tensor inside the flat training buffers

// One axis of a weight's natural layout as a list of (logical, physical) segment lengths: when the caller's hidden width
// is below the narrowest instantiated recurrent tile (dims.H = 16 or 32, the reference's own default d_dim = 16,
// train.py:85), the kernels run at a physical width of 64 with the extra hidden units' weights, biases and initial state
// exactly zero -- such a unit stays at 0 for ever (c = tanh(0) = 0, h' = u*0 + (1-u)*0) and feeds nothing, and the
// added products are exact zeros, so the logical units' values do not change.
struct EmbedAxis { std::vector<std::pair<int, int>> seg; };
struct Embed { EmbedAxis rows, cols; };

struct desire_ctx {
    desire_dims d;                                           // d.H is the PHYSICAL hidden width the kernels run at
    int Hl = 0;                                              // logical hidden width = dims.H as given to desire_create
    int A, R, V, B, E;
    std::map<std::string, size_t> want_user;                 // name -> element count in the caller's (logical) layout
    std::map<std::string, Embed> emb;                        // weights whose logical layout differs from the physical one
    std::map<std::string, std::vector<float>> host_w;       // raw weights as set
    std::map<std::string, size_t> want;                      // name -> element count
    Workspace dev{dev_malloc, dev_free};                     // raw / packed / folded device tensors (workspace.h)
    Workspace ws{dev_malloc, dev_free};                      // workspace
    bool finalized = false;
    std::vector<void*> graphs;                               // instantiated hipGraphExec_t of desire_graph_end
    std::vector<float> bin_tab_host;                         // log-polar bin table (20 floats) when dims.bin_mode == 1
    const float* grids = nullptr;
    bool grids_set = false;
    bool profiling = false;
    // peer exchange of the agent-sharded IOC (desire_peer_*): this rank's region, the mapped regions of the others, a mapped host error word
    void* peer_region = nullptr; size_t peer_bytes = 0; void* peer_base[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool peer_mapped[8] = {false, false, false, false, false, false, false, false}; int peer_rank = -1, peer_nranks = 0; bool peer_ready = false;
    int* peer_err = nullptr;
    float head_loss_w = 0.f;                                 // desire_set_head_loss: weight of the Gaussian-head NLL term in the training loss
    int recon_mode = 0; float recon_tau = 0.f;               // desire_set_recon_loss: DESIRE_RECON_* of the training loss's reconstruction term, the soft-min temperature
    int recon_scope = 0;                                     // desire_set_recon_scope: DESIRE_RECON_SCOPE_* (per agent, or per window over its K worlds)
    float col_w = 0.f, col_radius = 0.f, col_ux = 1.f, col_uy = 1.f;      // desire_set_collision_loss: weight (0 = off), radius and unit of the training loss's collision term
    // desire_set_offroad_field / desire_set_offroad_loss: the caller's distance fields (referenced, not copied; nullptr: none set) with their shape,
    // the weight (0 = off) and the scale of the training loss's off-road term; the window -> field map is the workspace's "off_fos"
    const float* off_field = nullptr; int off_n = 0, off_Mh = 0, off_Mw = 0; float off_w = 0.f, off_scale = 0.f;
    // desire_set_refined_loss: the same three terms on the refined trajectories "Y_ref" -- the regression term follows the recon mode and scope (0: the
    // plain mean), the weights of the collision and the off-road term there (0 = off; radius, units, field and scale are the ones above)
    int ref_recon = 0; float rcol_w = 0.f, roff_w = 0.f;
    int* host_err = nullptr;                                 // mapped host word the bin-split IOC's bounded spins report into (checked by the next call)
    // present-row compaction (DESIRE_FLAG_COMPACT_ROWS, kernels_compact.hip): mapped host word the scan kernel reports the present-agent count
    // into, the event behind it, the count of the last desire_sample (-1: none yet)
    int32_t* cp_host = nullptr; hipEvent_t cp_ev = nullptr; bool cp_pending = false; int cp_P = -1;
    int ci_cnt[4] = {0, 0, 0, 0}; bool ci_last = false; int ci_min_rows = 8192;     // DESIRE_FLAG_COMPACT_IOC: windows per slot class of the last IOC stage
    bool cp_enc = false;                                     // the last desire_encode ran its stack on the present agents only (saves in compact agent order)
    bool cp_host_counts = false;                             // desire_set_option("compact_host_counts", 1): inference reads the counts back like training does (A/B)
    bool cp_last = false;                                    // the last desire_sample ran compacted (desire_backward follows it, not the flag)
    int scene_modes_chunk = 0;                               // desire_set_option("scene_modes_chunk", c): desire_fit_scene_modes walks at most c slots per chunk (0: what the LDS holds; the tests' lever)
    // desire_build_windows*: plain pointers, cached at creation -- a feeder thread may run the builder while the owner thread runs a forward or a backward on
    // the same handle (desire_amd/prefetch.py: DeviceWindowFeeder), and those allocate workspace entries lazily (allocation inserts; reads do not): the
    // builder must not walk the map
    int32_t* bw_starts = nullptr; int32_t* bw_err = nullptr;
    // desire_set_rng: the generator's device words "rng_state" (next, used, seed_lo, seed_hi; nullptr = off) and the origin of desire_set_rng_origin
    uint32_t* rng_state = nullptr; uint32_t rng_scene_base = 0, rng_slot_base = 0;
    std::vector<Prof> prof;
    std::vector<std::string> prof_name_store;
    // ---- training (train.hip) ----
    bool training = false;
    std::map<std::string, WSlot> slots;                      // natural-layout offsets in Wflat / Gflat / Mflat / Vflat
    size_t n_params = 0;
    const float* last_eps = nullptr;                         // inputs of the last training-mode forward
    int adam_t = 0;                                          // Adam step counter
    int n_seg = 0;                                           // repack segments (train.hip)
    int n_seg16 = 0;                                         // split [hi | lo] bf16 packs among them (dims.bf16 = 2)
    bool scene_grad = false;                                 // desire_set_option(h, "scene_grad", 1): desire_backward also writes "scene_grid_grad"
    // desire_set_scene_images: the handle runs the scene CNN itself into its own grid buffer "scene_img_grid" (scnn1 / scnn2 kept for the backward)
    const float* img = nullptr; bool img_set = false;        // (desire_set_scene_grids detaches them: the last setter called wins)
    bool img_stale = true;                                   // the grid does not reflect the current weights / images (inference reruns the CNN)
};

struct Timer {
    desire_ctx* h; hipStream_t s; bool on; size_t idx = 0;        // idx: its own entry (a Timer may run inside another one)
    Timer(desire_ctx* h_, hipStream_t s_, const char* name) : h(h_), s(s_), on(h_->profiling) {
        if (!on) return;
        Prof p; p.name = name;
        (void)hipEventCreate(&p.e0); (void)hipEventCreate(&p.e1);
        (void)hipEventRecord(p.e0, s);
        idx = h->prof.size();
        h->prof.push_back(p);
    }
    ~Timer() { if (on) (void)hipEventRecord(h->prof[idx].e1, s); }
};

// the kernel forms of sample generation and of the matching parts of the training step, for the handle as it stands (gen_plan.h)
inline GenPlan gen_plan(const desire_ctx* h) { return gen_plan(h->d, h->training, h->V); }

// Lookups by name: nullptr for a name that was never allocated (workspace.h: they neither insert nor throw)
inline const float* D(desire_ctx* h, const char* name) { return h->dev.get(name); }
inline const float4* D4(desire_ctx* h, const char* name) { return h->dev.get<const float4>(name); }
inline float* W(desire_ctx* h, const char* name) { return h->ws.get(name); }
template <class T> T* Wt(desire_ctx* h, const char* name) { return h->ws.get<T>(name); }      // the non-float workspace buffers
// every buffer of a list (workspace.h: ensure_all); a failure is reported by name
template <size_t N> int ws_ensure(desire_ctx* h, const WsItem (&list)[N]) {
    std::string failed;
    return h->ws.ensure_all(list, N, &failed) ? fail(DESIRE_ERR_HIP, "hipMalloc failed for " + failed) : 0;
}

// logical (caller) layout <-> physical layout of one named weight (identity when the weight has no Embed entry)
std::vector<float> desire_embed(const desire_ctx* h, const std::string& name, const float* user);
void desire_extract(const desire_ctx* h, const std::string& name, const float* phys, float* user);
int desire_upload(desire_ctx* h, const std::string& name, const std::vector<float>& v);
int desire_ready(desire_handle* h);
bool compact_rows(const desire_ctx* h);                        // DESIRE_FLAG_COMPACT_ROWS set
bool compact_ioc(const desire_ctx* h);                         // DESIRE_FLAG_COMPACT_IOC set and the shape is served
bool compact_dyn(const desire_ctx* h);                         // compacted launches take their counts from device words (inference, frozen batch-norm): no host wait
int compact_setup(desire_ctx* h);                              // its buffers, event and mapped count word (idempotent)
inline IocPlan ioc_plan(const desire_ctx* h) { return ioc_plan(h->d, h->training, h->d.mno, 0, h->R); }     // of the handle's own shape (ioc_plan.h)
// A view of the handle's rows that one IOC launch sequence -- the forward or its BPTT -- runs on: the handle's own layout (cls = -1), or one
// slot class of DESIRE_FLAG_COMPACT_IOC, n_scenes windows of mno slots seated in the class buffers at the class's offsets
struct IocView {
    int cls = -1, mno = 0, n_scenes = 0, gpt = 0, ngrp = 0;  // gpt, ngrp: padded tiles (kernels.h: IocArgs.gpt); R = tiles * 32
    long R = 0;
    size_t agent_off = 0, row_off = 0, win_off = 0;          // in ci_Hx / ci_pl / ci_valid, in ci_Y / ci_score and the training saves, in ci_gos
    float* Hx = nullptr; float* p_last = nullptr; uint8_t* valid = nullptr; int32_t* gos = nullptr;     // agent-level inputs (Hx: ld 2H)
    const int32_t* cmap = nullptr; const int32_t* win = nullptr;                                        // a slot class's agent map and windows
    float* Y = nullptr; float* score = nullptr; const int32_t* dynN = nullptr;     // forward: its rows; device-side counts: the class's window count
};
// The slot classes (ascending, the handle's mno last; class 10 only when `pad`) with their geometry and offsets for per-class window counts
// (nullptr: the worst case, every window in every class -- device-side counts and buffer sizing)
struct ClassLayout { int n = 0; int m[4] = {0, 0, 0, 0}; IocView c[4]; size_t agents = 0, rows = 0, wins = 0; };
ClassLayout class_layout(const desire_ctx* h, bool pad, const int* counts);
IocView ioc_view(desire_ctx* h, const IocView* cls = nullptr);     // a class of class_layout with its pointers bound; nullptr: the handle's own layout
// Rows of the IOC buffers: the handle's rows + slack for the partial padded tiles of the slot classes (DESIRE_FLAG_COMPACT_IOC).  The training-mode
// forward (ioc_core) writes each refinement pass's saves and the backward reads them at ioc_save_off, in (row, t) units: a pass's stride is
// ioc_save_rows * T_pred, a view's saves start at its row offset.
inline size_t ioc_save_rows(const desire_ctx* h) { return (size_t)h->R + 128; }
inline size_t ioc_save_off(const desire_ctx* h, int pass, const IocView& v) { return ((size_t)pass * ioc_save_rows(h) + v.row_off) * h->d.T_pred; }
// The cluster form's exchange, sized for the handle's own shape (every view is smaller): allocated on first use, the counters of n_groups groups
// zeroed (and the error word when reset_err); ioc_cluster_check reads the error word back (a stream synchronisation)
int ioc_cluster_exchange(desire_ctx* h, size_t n_groups, bool reset_err, hipStream_t s);
int ioc_cluster_check(desire_ctx* h, hipStream_t s, const char* what);
void ioc_timing_report(const long long* dbg, const char* const* names, int n, hipStream_t s);      // DESIRE_IOC_TIMING: per-phase cycle counters -> stderr
int desire_pack_all(desire_ctx* h);                            // (re)builds every device operand of pack.h's table from host_w
int scene_grad_setup(desire_ctx* h);                           // buffers of the scene-grid gradient (train.hip; idempotent, training mode only)
inline bool scene_grad_on(const desire_ctx* h) { return h->scene_grad || h->img_set; }      // images attached imply the grid gradient
void enc_weights(desire_ctx* h, const char* prefix, EncArgs& e);     // the fp32 GRU weights of the encoder "enc_x" / "enc_y" (api_forward.hip)
IocStepArgs ioc_step_args(desire_ctx* h, int t);               // what every launch of the step-wise IOC kernel shares (api_peer.hip)
inline RngArgs rng_args(const desire_ctx* h) { return RngArgs{h->rng_state, 0u, 0u, 0u, h->rng_scene_base, h->rng_slot_base}; }      // the handle's generator
int recon_ws_setup(desire_ctx* h);                             // "recon_e" / "recon_w" / "recon_win" / "recon_val" (api_eval.hip; idempotent)
int recon_scene_ws_setup(desire_ctx* h);                       // those four and "recon_E" / "recon_cnt" of the scene scope (api_eval.hip; idempotent)
// Where a term of the training step reads and writes, by workspace tensor name: the sample tensor, the gradient it adds to, its outputs.  Two targets
// each: the decoder's samples "Y0" with "dY0" (backward.hip: loss_grads) and the refined trajectories "Y_ref" with "dYr" (ioc_bwd), whose outputs are
// tensors of their own (r*) so that neither side overwrites what the other left.
struct ReconTarget { const char *Y, *e, *w, *win, *val, *E, *cnt; };
struct TermTarget { const char *Y, *dY, *val, *count, *term; float weight; };
constexpr ReconTarget RECON_Y0{"Y0", "recon_e", "recon_w", "recon_win", "recon_val", "recon_E", "recon_cnt"};
constexpr ReconTarget RECON_REFINED{"Y_ref", "rrecon_e", "rrecon_w", "rrecon_win", "rrecon_val", "rrecon_E", "rrecon_cnt"};
inline TermTarget col_target_y0(const desire_ctx* h) { return TermTarget{"Y0", "dY0", "col_val", "col_touch", "col_term", h->col_w}; }
inline TermTarget col_target_refined(const desire_ctx* h) { return TermTarget{"Y_ref", "dYr", "rcol_val", "rcol_touch", "rcol_term", h->rcol_w}; }
inline TermTarget off_target_y0(const desire_ctx* h) { return TermTarget{"Y0", "dY0", "off_val", "off_count", "off_term", h->off_w}; }
inline TermTarget off_target_refined(const desire_ctx* h) { return TermTarget{"Y_ref", "dYr", "roff_val", "roff_count", "roff_term", h->roff_w}; }
// the reconstruction weights of the training step into the target's workspace tensors, in the handle's mode and scope (api_eval.hip; mode != MEAN)
void recon_weights_enqueue(desire_ctx* h, const ReconTarget& tg, const float* fut, const uint8_t* lmask, hipStream_t s);
int collision_ws_setup(desire_ctx* h);                         // "col_val" / "col_touch" / "col_grad" / "col_term" and "nvalid" (api_eval.hip; idempotent)
int check_collision_args(float radius, float unit_x, float unit_y);      // desire_collision_loss' checks of its scalars (api_eval.hip)
// the collision term of the training step: dY = dY + weight * G in place, col, touch and the term into the target's tensors (api_eval.hip; weight > 0)
void collision_enqueue(desire_ctx* h, const TermTarget& tg, const float* fut, const uint8_t* lmask, hipStream_t s);
int offroad_ws_setup(desire_ctx* h);                           // "off_val" / "off_count" / "off_grad" / "off_term" and "nvalid" (api_eval.hip; idempotent)
// the off-road term of the training step: dY = dY + weight * G in place, off, count and the term into the target's tensors (api_eval.hip; weight > 0)
void offroad_enqueue(desire_ctx* h, const TermTarget& tg, const float* fut, const uint8_t* lmask, hipStream_t s);
// the refined side's workspace (desire_set_refined_loss): the six "rrecon_*" with recon, "rcol_*" / "roff_*" with their weights (api_eval.hip; idempotent)
int refined_ws_setup(desire_ctx* h, bool recon, bool collision, bool offroad);
int scene_images_run(desire_ctx* h, hipStream_t s);            // the scene CNN over the attached images into "scene_img_grid" (api_ops.hip)
