// eval_lds.h -- the dynamic-LDS plans of the evaluation kernels over the sample tensor Y [R, T_pred, 2] (kernels_rank / _kde / _select / _joint /
// _recon / _occ / _plan / _plan_cond / _modes / _worlds / _scene_modes / _collision / _offroad.hip): the one budget, the one workgroup size, and per kernel a plan (its regions in order, with their offsets and bytes()) and the geometry
// that picks the plan's parameters.  The geometry, the launcher's LDS argument and the kernel's carve-up all go through the plan.
// Plain C++ without HIP headers: tests/c_host/eval_lds_driver.cpp, occ_lds_driver.cpp, scene_modes_lds_driver.cpp, plan_cond_lds_driver.cpp, coll_lds_driver.cpp and offroad_lds_driver.cpp compile it with g++
// (tests/test_eval_lds.py, test_occ_lds.py, test_scene_modes_cpu.py, test_plan_cond_cpu.py, test_collision_cpu.py, test_offroad_cpu.py).
#pragma once
#include <stddef.h>

#include "../../include/desire_hip.h"           // DESIRE_DIST_FINAL

#ifdef __HIPCC__
#define EVAL_HD __host__ __device__
#else
#define EVAL_HD
#endif

constexpr int EVAL_THREADS = 256;               // lanes of a workgroup of every streaming kernel
constexpr int EVAL_LDS_BYTES = 60 * 1024;       // dynamic LDS of a workgroup (below the 64 KiB a launch gets without asking for more)
constexpr int EVAL_PAIR_BYTES = 8;              // a position: float2
// in a kernel: one clause tying an element type of its carve-up to the plan its launcher sizes the LDS by
#define EVAL_LDS_TIED(cond) static_assert(cond, "carve-up and eval_lds.h plan disagree: " #cond)

EVAL_HD constexpr int eval_min(int a, int b) { return a < b ? a : b; }
EVAL_HD constexpr int eval_max(int a, int b) { return a > b ? a : b; }
EVAL_HD constexpr int eval_odd(int n) { return n | 1; }                 // row stride of n frames: odd, so a walk down the rows is bank-conflict free
EVAL_HD constexpr int eval_chunks(int n, int per) { return (n + per - 1) / per; }

// ---- k_sample_errors: floats.  gm, gx, gy [SC][Tp] (counted mask and targets of the slot chunk), e [KC * SC][Tp] (the errors of the chunk's rows)
struct ErrLds {
    int Tp, SC, KC;
    EVAL_HD constexpr ErrLds(int T, int SC_, int KC_) : Tp(eval_odd(T)), SC(SC_), KC(KC_) {}
    EVAL_HD constexpr int gm() const { return 0; }
    EVAL_HD constexpr int gx() const { return SC * Tp; }
    EVAL_HD constexpr int gy() const { return 2 * SC * Tp; }
    EVAL_HD constexpr int e() const { return 3 * SC * Tp; }
    EVAL_HD constexpr size_t bytes() const { return 4 * (size_t)Tp * ((size_t)3 * SC + (size_t)SC * KC); }
};
// The chunking: every slot of a window and as many samples as 256 rows hold, shrunk until the LDS fits; the samples are then spread evenly over
// the chunks.  false: not even one row fits (T_pred beyond ~3800).
inline bool sample_errors_geometry(int mno, int K, int T, int* SC, int* KC) {
    int sc = mno, kc = eval_max(1, eval_min(K, EVAL_THREADS / sc));
    auto over = [&] { return ErrLds(T, sc, kc).bytes() > (size_t)EVAL_LDS_BYTES; };
    while (over() && kc > 1) kc = (kc + 1) / 2;
    while (over() && sc > 1) sc = (sc + 1) / 2;
    if (over()) return false;
    *SC = sc; *KC = eval_chunks(K, eval_chunks(K, kc));
    return true;
}

// ---- k_kde_nll: floats.  val, cm [SA][Tp] (frame value and counted mask of SA whole agents)
struct KdeLds {
    int Tp, SA;
    EVAL_HD constexpr KdeLds(int T, int SA_) : Tp(eval_odd(T)), SA(SA_) {}
    EVAL_HD constexpr int val() const { return 0; }
    EVAL_HD constexpr int cm() const { return SA * Tp; }
    EVAL_HD constexpr size_t bytes() const { return (size_t)SA * (size_t)Tp * 8; }
};
// Whole agents per workgroup: as many as 256 (agent, t) pairs hold, one when T_pred is longer than that (the lanes then loop over its frames).
// false: one agent's T_pred frame values do not fit.
inline bool kde_geometry(int T, int* SA) {
    const int sa = eval_max(1, EVAL_THREADS / T);
    if (KdeLds(T, sa).bytes() > (size_t)EVAL_LDS_BYTES) return false;
    *SA = sa;
    return true;
}

// ---- k_select_diverse: Yl float2 [SC][K][Tp] (Tp = staged frames | 1), then five [SC][K] words (input order, candidate state, weight, order out,
// mass), then two [SC] words (count, range flag).  The limit this gives is stated in desire_hip.h and in desire_select_diverse's message.
struct SelLds {
    enum { K_WORDS = 5, SLOT_WORDS = 2 };
    int Tp, SC, K;
    EVAL_HD static constexpr int staged(int metric, int t_end) { return metric == DESIRE_DIST_FINAL ? 1 : t_end; }
    EVAL_HD constexpr SelLds(int staged_, int SC_, int K_) : Tp(eval_odd(staged_)), SC(SC_), K(K_) {}
    EVAL_HD constexpr size_t pairs() const { return (size_t)SC * K * Tp; }                  // float2 in front of the words
    EVAL_HD constexpr int k_words(int r) const { return r * SC * K; }                       // region r of the [SC][K] words, in words behind the pairs
    EVAL_HD constexpr int slot_words(int r) const { return K_WORDS * SC * K + r * SC; }     // region r of the [SC] words
    EVAL_HD static constexpr size_t agent_bytes(int K, int staged_) {
        return (size_t)K * (EVAL_PAIR_BYTES * (size_t)eval_odd(staged_) + 4 * K_WORDS) + 4 * SLOT_WORDS;
    }
    EVAL_HD constexpr size_t bytes() const { return (size_t)SC * agent_bytes(K, Tp); }     // (Tp | 1 == Tp)
};
// The slot chunk: as many agents as the LDS holds, no more than 256 / G * 2 (two agents per group of G lanes keep the tail short), spread evenly over
// the chunks; G = the power of two >= K, 64 at most.  false: one agent does not fit.
inline bool select_geometry(int mno, int K, int metric, int t_end, int* SC, int* G) {
    const size_t per = SelLds::agent_bytes(K, SelLds::staged(metric, t_end));
    if (per > (size_t)EVAL_LDS_BYTES) return false;
    int g = 1;
    while (g < K && g < 64) g <<= 1;
    int sc = (int)((size_t)mno < (size_t)EVAL_LDS_BYTES / per ? (size_t)mno : (size_t)EVAL_LDS_BYTES / per);
    sc = eval_min(sc, eval_max(1, 2 * EVAL_THREADS / g));
    *SC = eval_chunks(mno, eval_chunks(mno, sc));
    *G = g;
    return true;
}

// ---- k_recon_weights: Yl float2 [KC][SC][Tp] (the rows of a pass), gl float2 [SC][Tp] (targets), cl int [SC][Tp] (frame t of the slot counts)
struct ReconLds {
    int Tp, SC, KC;
    EVAL_HD constexpr ReconLds(int T, int SC_, int KC_) : Tp(eval_odd(T)), SC(SC_), KC(KC_) {}
    EVAL_HD constexpr size_t rows() const { return (size_t)KC * SC * Tp; }                  // float2 in front of the targets
    EVAL_HD constexpr size_t slots() const { return (size_t)SC * Tp; }                      // float2 of the targets, and ints of the flags behind them
    EVAL_HD static constexpr size_t row_bytes(int T) { return EVAL_PAIR_BYTES * (size_t)eval_odd(T); }
    EVAL_HD static constexpr size_t slot_bytes(int T) { return (EVAL_PAIR_BYTES + 4) * (size_t)eval_odd(T); }
    EVAL_HD constexpr size_t bytes() const { return (size_t)KC * SC * row_bytes(Tp) + (size_t)SC * slot_bytes(Tp); }
};
// The slot chunk and the samples of a pass: as many rows as the LDS holds next to their slots' targets, 256 at most (one lane per row), all K samples
// of a slot in one pass where that fits (then more, smaller workgroups), the slots spread evenly over the chunks.  false: one row with its targets
// does not fit (T_pred beyond 3071).
inline bool recon_geometry(int mno, int K, int T, int* SC, int* KC) {
    const size_t per = ReconLds(T, 1, 1).bytes();                      // a row with a slot of its own: the bound below holds for every SC x KC <= cap
    if (per > (size_t)EVAL_LDS_BYTES) return false;
    const int cap = (int)((size_t)EVAL_THREADS < (size_t)EVAL_LDS_BYTES / per ? (size_t)EVAL_THREADS : (size_t)EVAL_LDS_BYTES / per);
    const int sc = eval_min(mno, eval_max(1, cap / K));
    *SC = eval_chunks(mno, eval_chunks(mno, sc));
    *KC = eval_min(K, eval_max(1, cap / *SC));
    return true;
}

// ---- k_joint_unit: P float2 [TC][mp] (frame stride mp = mno below 32 slots, mno + 1 from 32 on: kernels_joint.hip says why), then two [mno] ints
// (first contact, first counted frame)
struct JointLds {
    int mno, TC;
    EVAL_HD constexpr JointLds(int mno_, int TC_) : mno(mno_), TC(TC_) {}
    EVAL_HD static constexpr int stride(int mno) { return mno >= 32 ? mno + 1 : mno; }
    EVAL_HD constexpr size_t pairs() const { return (size_t)TC * stride(mno); }             // float2 in front of the ints
    EVAL_HD constexpr size_t bytes() const { return pairs() * EVAL_PAIR_BYTES + (size_t)mno * 2 * 4; }
};
// Frames per chunk: the whole horizon when mno * T_pred positions and the two per-slot integers fit the plan, else as many frames as do.  One
// frame of 256 slots is 2 KB, so every (mno, T_pred) a handle can have is served.
inline int joint_chunk_frames(int mno, int T) {
    const size_t fixed = JointLds(mno, 0).bytes(), per = JointLds(mno, 1).bytes() - fixed, fit = ((size_t)EVAL_LDS_BYTES - fixed) / per;
    return (int)((size_t)T < fit ? (size_t)T : fit);
}

// ---- k_collision_unit: P float2 [TC][mp] (the unit's positions, JointLds' layout and frame stride), Gl float2 [mno][eval_odd(TC)] (the gradient of
// the chunk's frames, parked slot-major so that it leaves in row order), then behind the pairs, in 32-bit words: Sl float [mno][eval_odd(TC)] (s(i, t),
// walked by one lane per slot in increasing t), two [mno] floats (1 / nfut of a counted slot or 0, the running sum of s carried across the
// chunks) and one int (the unit's touch count).  The odd row stride keeps the lanes of consecutive slots on distinct banks in both parks.
struct CollLds {
    enum { SLOT_WORDS = 2, UNIT_WORDS = 1 };
    int mno, TC;
    EVAL_HD constexpr CollLds(int mno_, int TC_) : mno(mno_), TC(TC_) {}
    EVAL_HD constexpr int park_stride() const { return eval_odd(TC); }
    EVAL_HD constexpr size_t pos() const { return (size_t)TC * JointLds::stride(mno); }     // float2 in front of the gradient park
    EVAL_HD constexpr size_t grad() const { return (size_t)mno * park_stride(); }           // float2 in front of the words
    EVAL_HD constexpr size_t s_words() const { return (size_t)mno * park_stride(); }        // word offsets behind the pairs: Sl at 0
    EVAL_HD constexpr size_t slot_words(int r) const { return s_words() + (size_t)r * mno; }
    EVAL_HD constexpr size_t unit_words() const { return slot_words(SLOT_WORDS); }
    EVAL_HD constexpr size_t bytes() const { return (pos() + grad()) * EVAL_PAIR_BYTES + 4 * (unit_words() + UNIT_WORDS); }
};
// Frames per chunk: the whole horizon when the unit fits, else the largest number of frames that does.  A frame costs 8 stride + 12 mno bytes and
// the odd park stride at most one more frame's worth of the parks: two frames of 256 slots are 15.4 KB with it, so every (mno, T_pred) a handle
// can have is served (11 frames at 256 slots).
inline int coll_chunk_frames(int mno, int T) {
    auto fits = [&](int tc) { return CollLds(mno, tc).bytes() <= (size_t)EVAL_LDS_BYTES; };
    if (fits(T)) return T;
    int tc = (int)(((size_t)EVAL_LDS_BYTES - CollLds(mno, 0).bytes()) / ((size_t)EVAL_PAIR_BYTES * JointLds::stride(mno) + (size_t)12 * mno));
    tc = eval_max(1, eval_min(tc, T));
    while (tc > 1 && !fits(tc)) --tc;              // (the estimate counts the odd stride's extra column once: a step or two either way)
    while (tc < T && fits(tc + 1)) ++tc;
    return tc;
}

// ---- k_offroad_unit: CollLds' regions in CollLds' order -- P float2 [TC][mp], Gl float2 [mno][eval_odd(TC)], then in words Sl [mno][eval_odd(TC)]
// (phi(i, t)), two [mno] floats (1 / nfut of a counted slot or 0, the running sum of phi) and one int (the unit's off-road count) -- and behind them
// F float [cells]: the window's distance field, cells = Mh * Mw when it is staged, 0 when the kernel gathers the taps from global memory.
struct OffLds {
    CollLds c;
    int cells;
    EVAL_HD constexpr OffLds(int mno_, int TC_, int cells_) : c(mno_, TC_), cells(cells_) {}
    EVAL_HD constexpr size_t field_words() const { return c.unit_words() + CollLds::UNIT_WORDS; }      // word offset of F behind the pairs
    EVAL_HD constexpr size_t bytes() const { return c.bytes() + (size_t)4 * cells; }
};
// The frames per chunk are CollLds' (a field never makes a unit walk more chunks); the field is staged when it fits behind that plan -- 64 x 64
// cells next to 32 slots x 40 frames do (42.9 KB), next to 256 slots x 11 frames they do not -- and is read from global memory otherwise.
inline void offroad_geometry(int mno, int T, int Mh, int Mw, int* TC, int* staged) {
    *TC = coll_chunk_frames(mno, T);
    *staged = OffLds(mno, *TC, Mh * Mw).bytes() <= (size_t)EVAL_LDS_BYTES ? 1 : 0;
}

// ---- k_plan_risk: PL float2 [PC][eval_odd(TC)] (the frames of a pass of a chunk of PC candidate plans), P float2 [TC][mp] (the unit's positions,
// JointLds' layout and frame stride), then two sets -- one per parity of k -- of PC ints (first contact of the plan with any slot) and PC * HZ
// words (its clearance per horizon: the bits of a non-negative float, which order as unsigned integers)
struct PlanLds {
    enum { HZ = 8, MAX_PC = EVAL_THREADS / HZ, SETS = 2 };                 // one lane per (plan, horizon) keeps the risk: PC * HZ <= EVAL_THREADS
    int mno, PC, TC;
    EVAL_HD constexpr PlanLds(int mno_, int PC_, int TC_) : mno(mno_), PC(PC_), TC(TC_) {}
    EVAL_HD constexpr int plan_stride() const { return eval_odd(TC); }
    EVAL_HD constexpr size_t plans() const { return (size_t)PC * plan_stride(); }           // float2 in front of the positions
    EVAL_HD constexpr size_t pos() const { return (size_t)TC * JointLds::stride(mno); }     // float2 in front of the words
    EVAL_HD constexpr int first(int set) const { return set * PC * (1 + HZ); }              // word offsets behind the pairs
    EVAL_HD constexpr int clear(int set) const { return first(set) + PC; }
    EVAL_HD constexpr size_t bytes() const { return (plans() + pos()) * EVAL_PAIR_BYTES + (size_t)4 * first(SETS); }
};
// The plan chunk: as many plans as EVAL_THREADS (plan, slot) items hold -- every lane owns one item for the whole call -- MAX_PC at most, spread
// evenly over the chunks of the M plans.  Frames per pass: the whole horizon when the chunk's plans and the unit's positions fit, else as many
// frames of both as do (eval_odd(TC) <= TC + 1).  One frame of 256 slots and one plan is 2 KB, so every (mno, T_pred, M) is served.
inline void plan_geometry(int mno, int T, int M, int* PC, int* TC) {
    const int cap = eval_min(eval_min(M, (int)PlanLds::MAX_PC), eval_max(1, EVAL_THREADS / mno));
    const int pc = eval_chunks(M, eval_chunks(M, cap));
    const size_t fixed = PlanLds(mno, pc, 0).bytes(), per = (size_t)EVAL_PAIR_BYTES * ((size_t)pc + JointLds::stride(mno));
    const size_t fit = ((size_t)EVAL_LDS_BYTES - fixed) / per;            // (PlanLds(.., 0) already holds the one pair per plan of the odd stride)
    *PC = pc;
    *TC = (int)((size_t)T < fit ? (size_t)T : fit);
}

// ---- k_plan_cond_weights: PL float2 [PC][eval_odd(TC)] (the compared frames of a pass of a chunk of PC candidate plans, PlanLds' row stride),
// then, when rows_in_lds, E float2 [K][eval_odd(TC)] (the K rows of the ONE ego slot the chunk's plans name), then two [PC] ints (the ego slot of
// a plan or -1, its compared frames so far).  Nothing else grows with K: the K distances and weight numerators of a plan are parked in the
// call's own output dev_cw, so every K is served.
struct PlanCondLds {
    enum { MAX_PC = 64, ITEMS = 4 * EVAL_THREADS, PLAN_WORDS = 2 };       // a lane owns ITEMS / EVAL_THREADS (plan, k) items at most where M allows
    int K, PC, TC, rows_in_lds;
    EVAL_HD constexpr PlanCondLds(int K_, int PC_, int TC_, int rows_) : K(K_), PC(PC_), TC(TC_), rows_in_lds(rows_ ? 1 : 0) {}
    EVAL_HD constexpr int stride() const { return eval_odd(TC); }
    EVAL_HD constexpr size_t plans() const { return (size_t)PC * stride(); }                // float2 in front of the ego rows
    EVAL_HD constexpr size_t rows() const { return rows_in_lds ? (size_t)K * stride() : 0; }     // float2 in front of the words
    EVAL_HD constexpr int ego() const { return 0; }                                         // word offsets behind the pairs
    EVAL_HD constexpr int count() const { return PC; }
    EVAL_HD constexpr size_t bytes() const { return (plans() + rows()) * EVAL_PAIR_BYTES + (size_t)4 * PLAN_WORDS * PC; }
};
// The plan chunk: as many plans as ITEMS (plan, k) items hold, MAX_PC at most, spread evenly over the chunks of the M plans.  The frames are the
// t_cond compared ones.  When the chunk's plans and the K ego rows fit, both are staged whole (rows = 1).  Else the rows stay in global memory
// (rows = 0) and the plans are staged whole, or -- beyond ~7600 frames of one plan -- in passes of TC frames: 16 PC bytes are fixed and a frame
// of the chunk is 8 PC <= 512 bytes, so every (K, t_cond, M) is served.
inline void plan_cond_geometry(int K, int t_cond, int M, int* PC, int* TC, int* rows) {
    const int cap = eval_min(eval_min(M, (int)PlanCondLds::MAX_PC), eval_max(1, (int)PlanCondLds::ITEMS / K));
    const int pc = eval_chunks(M, eval_chunks(M, cap));
    *PC = pc;
    if (PlanCondLds(K, pc, t_cond, 1).bytes() <= (size_t)EVAL_LDS_BYTES) { *TC = t_cond; *rows = 1; return; }
    const size_t fixed = PlanCondLds(K, pc, 0, 0).bytes(), per = (size_t)EVAL_PAIR_BYTES * pc;
    const size_t fit = ((size_t)EVAL_LDS_BYTES - fixed) / per;            // (PlanCondLds(.., 0, 0) already holds the one pair per plan of the odd stride)
    *TC = (int)((size_t)t_cond < fit ? (size_t)t_cond : fit);
    *rows = 0;
}

// ---- k_fit_modes: float2 rows Yl [SC][K][Tp] (all T frames of the K samples of SC agents, Tp = T | 1), then the running means ml [SC][n][Tp] with
// the same stride; behind the pairs, in 32-bit words: cov float [SC][n][T][3] (Cxx, Cyy, Cxy: the layout of the output, so it leaves by a linear
// copy), val and cm float [SC][Tp] each (frame value and counted mask: KdeLds' pair), three [SC][K] words (weight, label, previous label), two
// [SC][n] words (mass, member count) and four [SC] words (bad order row, passes, and the two parities of `a label changed in the last assign`).
// The limit this gives is stated in desire_hip.h and in desire_fit_modes' message.
struct ModesLds {
    enum { FRAME_WORDS = 2, K_WORDS = 3, MODE_WORDS = 2, SLOT_WORDS = 4 };
    int T, Tp, SC, K, n;
    EVAL_HD constexpr ModesLds(int T_, int SC_, int K_, int n_) : T(T_), Tp(eval_odd(T_)), SC(SC_), K(K_), n(n_) {}
    EVAL_HD constexpr size_t rows() const { return (size_t)SC * K * Tp; }                   // float2 in front of the means
    EVAL_HD constexpr size_t pairs() const { return (size_t)SC * (K + n) * Tp; }            // float2 in front of the words
    EVAL_HD constexpr size_t cov() const { return 0; }                                      // word offsets behind the pairs
    EVAL_HD constexpr size_t frame_words(int r) const { return (size_t)3 * SC * n * T + (size_t)r * SC * Tp; }
    EVAL_HD constexpr size_t k_words(int r) const { return frame_words(FRAME_WORDS) + (size_t)r * SC * K; }
    EVAL_HD constexpr size_t mode_words(int r) const { return k_words(K_WORDS) + (size_t)r * SC * n; }
    EVAL_HD constexpr size_t slot_words(int r) const { return mode_words(MODE_WORDS) + (size_t)r * SC; }
    EVAL_HD static constexpr size_t agent_bytes(int K, int T, int n) {
        return EVAL_PAIR_BYTES * (size_t)(K + n) * eval_odd(T) + 4 * ((size_t)3 * n * T + (size_t)FRAME_WORDS * eval_odd(T) + (size_t)K_WORDS * K +
                                                                      (size_t)MODE_WORDS * n + SLOT_WORDS);
    }
    EVAL_HD constexpr size_t bytes() const { return (size_t)SC * agent_bytes(K, T, n); }
};
// The slot chunk: as many agents as the LDS holds, no more than one per group of G lanes (G = the power of two >= K, 64 at most, as in
// select_geometry; beyond 64 samples a group's lanes loop), spread evenly over the chunks.  false: one agent does not fit.
inline bool modes_geometry(int mno, int K, int T, int n, int* SC, int* G) {
    const size_t per = ModesLds::agent_bytes(K, T, n);
    if (per > (size_t)EVAL_LDS_BYTES) return false;
    int g = 1;
    while (g < K && g < 64) g <<= 1;
    int sc = (int)((size_t)mno < (size_t)EVAL_LDS_BYTES / per ? (size_t)mno : (size_t)EVAL_LDS_BYTES / per);
    sc = eval_min(sc, eval_max(1, EVAL_THREADS / g));
    *SC = eval_chunks(mno, eval_chunks(mno, sc));
    *G = g;
    return true;
}

// ---- k_fit_scene_modes: one workgroup owns a window and walks its taking-part slots in chunks of SC.  Per chunk, float2 rows Yl [SC][K][Tp] (all T
// frames of the K worlds' rows of the chunk's slots, Tp = T | 1) and the modes' means ml [SC][n][Tp] with the same stride; behind the pairs, in
// 32-bit words: three [SC][n][T] words of the last pass (a slot's quadratic term over its determinant, half the log of the determinant, and the
// state of (slot, mode, t): not counted / usable / not usable), ds [K * n][SC | 1] (the chunk's distances d_s; the odd stride keeps the lanes
// that each reduce one (world, mode) on distinct banks) and, kept across the chunks, D [K][n] (the running sum of d_s in increasing slot), three
// [K] words (weight, label, previous label), five [n] words (mass, the mass the mean was divided by, members, seed, `the mode has had mass`),
// member [n][ceil(K / 32)] (bit k: world k is one of the worlds the mode's mean is formed from), two [n][T] words (the running log-likelihood
// L_i of a frame and `usable so far`), three [T] words (slots counted, the frame's value, counted) and one [mno] word (the taking-part slots in
// increasing slot).  As in WorldsLds the chunks run over the SLOTS, never over the frames: what crosses a chunk border is a per-(world, mode)
// sum in increasing slot and a per-(mode, t) chain in increasing slot, so a chunked window has the bits of an unchunked one by construction.  A
// chunk's means are formed anew from the member words in every pass (a mode that lost its mass keeps the members its mean came from), so
// nothing per slot outlives its chunk.  The limit this gives is stated in desire_hip.h and in desire_fit_scene_modes' message.
struct SceneModesLds {
    enum { TERM_WORDS = 3, K_WORDS = 3, MODE_WORDS = 5, FRAME_WORDS = 2, T_WORDS = 3 };
    int T, Tp, SC, K, n, mno;
    EVAL_HD constexpr SceneModesLds(int T_, int SC_, int K_, int n_, int mno_) : T(T_), Tp(eval_odd(T_)), SC(SC_), K(K_), n(n_), mno(mno_) {}
    EVAL_HD static constexpr int member_words(int K) { return (K + 31) / 32; }
    EVAL_HD constexpr size_t rows() const { return (size_t)SC * K * Tp; }                   // float2 in front of the means
    EVAL_HD constexpr size_t pairs() const { return (size_t)SC * (K + n) * Tp; }            // float2 in front of the words
    EVAL_HD constexpr int ds_stride() const { return eval_odd(SC); }
    EVAL_HD constexpr size_t term(int r) const { return (size_t)r * SC * n * T; }           // word offsets behind the pairs
    EVAL_HD constexpr size_t ds() const { return term(TERM_WORDS); }
    EVAL_HD constexpr size_t dist() const { return ds() + (size_t)K * n * (SC + 1); }
    EVAL_HD constexpr size_t k_words(int r) const { return dist() + (size_t)K * n + (size_t)r * K; }
    EVAL_HD constexpr size_t mode_words(int r) const { return k_words(K_WORDS) + (size_t)r * n; }
    EVAL_HD constexpr size_t member() const { return mode_words(MODE_WORDS); }
    EVAL_HD constexpr size_t frame_words(int r) const { return member() + (size_t)n * member_words(K) + (size_t)r * n * T; }
    EVAL_HD constexpr size_t t_words(int r) const { return frame_words(FRAME_WORDS) + (size_t)r * T; }
    EVAL_HD constexpr size_t slots() const { return t_words(T_WORDS); }
    EVAL_HD static constexpr size_t fixed_bytes(int K, int T, int n, int mno) {
        return 4 * ((size_t)2 * K * n + (size_t)K_WORDS * K + (size_t)MODE_WORDS * n + (size_t)n * member_words(K) + (size_t)FRAME_WORDS * n * T +
                    (size_t)T_WORDS * T + (size_t)mno);
    }
    EVAL_HD static constexpr size_t slot_bytes(int K, int T, int n) {
        return EVAL_PAIR_BYTES * (size_t)(K + n) * eval_odd(T) + 4 * ((size_t)TERM_WORDS * n * T + (size_t)K * n);
    }
    EVAL_HD constexpr size_t bytes() const { return fixed_bytes(K, T, n, mno) + (size_t)SC * slot_bytes(K, T, n); }
};
// The slot chunk: as many slots as the LDS holds next to the per-window words, spread evenly over the chunks of mno.  false: the per-window words
// and one slot do not fit.  At (mno 32, K 20, T_pred 40, n 6) a chunk is 4 slots, at (256, 20, 40, 6) too.
inline bool scene_modes_geometry(int mno, int K, int T, int n, int* SC) {
    if (mno < 1 || K < 1 || T < 1 || n < 1) return false;
    const size_t fixed = SceneModesLds::fixed_bytes(K, T, n, mno), per = SceneModesLds::slot_bytes(K, T, n);
    if (fixed + per > (size_t)EVAL_LDS_BYTES) return false;
    const size_t fit = ((size_t)EVAL_LDS_BYTES - fixed) / per;
    const int sc = (int)((size_t)mno < fit ? (size_t)mno : fit);
    *SC = eval_chunks(mno, eval_chunks(mno, sc));
    return true;
}

// ---- k_occupancy: 32-bit words.  Over the `cells` of a band of grid rows: E, q, P floats (expected count, product of the complements, one
// agent's marginal) and, in mode UNTIL, S uint32 (the stamp of the last (agent, k) that reached the cell: `at most once per sample`).  Each is
// an array of its own, so the lanes of a wave that walk consecutive cells walk consecutive banks in every one of them, and E, q, P of one cell
// are never read by one instruction.  Behind them the staging of one chunk of an agent, `ent` = KC samples x FC frames: id int32 [ent] (the
// cell of a position, or a marker), then w float, off int, viol int [ent] (per sample of the chunk: its weight, `was off frame`, `visited a
// masked cell`; KC <= ent) and cm int [ent] (per frame of the chunk: counted; FC <= ent).
struct OccLds {
    enum { ENTRIES = 512, CHUNK_REGIONS = 5 };
    int cells, ent, until;
    EVAL_HD constexpr OccLds(int cells_, int ent_, int until_) : cells(cells_), ent(ent_), until(until_ ? 1 : 0) {}
    EVAL_HD static constexpr int cell_words(int until_) { return until_ ? 4 : 3; }
    EVAL_HD constexpr size_t E() const { return 0; }
    EVAL_HD constexpr size_t q() const { return (size_t)cells; }
    EVAL_HD constexpr size_t P() const { return (size_t)2 * cells; }
    EVAL_HD constexpr size_t S() const { return (size_t)3 * cells; }                        // (mode UNTIL only)
    EVAL_HD constexpr size_t chunk(int r) const { return (size_t)cell_words(until) * cells + (size_t)r * ent; }     // region r: id, w, off, viol, cm
    EVAL_HD constexpr size_t bytes() const { return 4 * chunk(CHUNK_REGIONS); }
};
// frames = the frames of a sample that one workgroup walks at most: 1 in mode AT, the largest horizon in mode UNTIL.  The chunk: all frames of
// as many samples as ENTRIES positions hold (spread evenly over the chunks), or part of one sample's frames when they are more than that.  The
// band: as many whole grid rows as the rest of the budget holds, spread evenly over the bands.  Ow <= 1024: one row always fits.
inline bool occupancy_geometry(int K, int frames, int Oh, int Ow, int until, int* KC, int* FC, int* rows) {
    if (K < 1 || frames < 1 || Oh < 1 || Ow < 1) return false;
    const int fc = eval_min(frames, (int)OccLds::ENTRIES);
    int kc = eval_min(K, eval_max(1, (int)OccLds::ENTRIES / fc));
    kc = eval_chunks(K, eval_chunks(K, kc));
    const size_t left = (size_t)EVAL_LDS_BYTES - OccLds(0, kc * fc, until).bytes();
    const size_t fit = left / (4 * (size_t)OccLds::cell_words(until)) / (size_t)Ow;
    if (fit < 1) return false;
    const int r = (size_t)Oh < fit ? Oh : (int)fit;
    *KC = kc; *FC = fc;
    *rows = eval_chunks(Oh, eval_chunks(Oh, r));
    return true;
}

// ---- k_select_worlds: Yk float2 [SC][Fp] (the staged frames of one kept world's rows of a chunk of SC taking-part slots, Fp = staged frames | 1,
// SelLds::staged's), then dv [K][SC | 1] words (candidate x slot of the chunk: the linear distance d_i, or the predicate near_i as an integer;
// the odd stride keeps the lanes that each reduce one candidate's slots on distinct banks), then nine [K] words (processing order, candidate
// state, weight, order out, mass, label, running sum D, running conjunction, the live list) and one [mno] word (the taking-part slots in
// increasing slot).  The chunks run over the SLOTS, never over the frames: a slot's value is finished inside its chunk and only the per-world
// reduction over the slots -- a sum in increasing slot, a conjunction -- is carried from chunk to chunk, so a chunked window has the bits of
// an unchunked one by construction.  The limit this gives is stated in desire_hip.h and in desire_select_worlds' message.
struct WorldsLds {
    enum { K_WORDS = 9 };
    int Fp, SC, K, mno;
    EVAL_HD constexpr WorldsLds(int staged_, int SC_, int K_, int mno_) : Fp(eval_odd(staged_)), SC(SC_), K(K_), mno(mno_) {}
    EVAL_HD constexpr size_t pairs() const { return (size_t)SC * Fp; }                      // float2 in front of the words
    EVAL_HD constexpr int dv_stride() const { return eval_odd(SC); }
    EVAL_HD constexpr size_t dv() const { return 0; }                                       // word offsets behind the pairs
    EVAL_HD constexpr size_t k_words(int r) const { return (size_t)K * (SC + 1) + (size_t)r * K; }
    EVAL_HD constexpr size_t slots() const { return k_words(K_WORDS); }
    EVAL_HD static constexpr size_t fixed_bytes(int K, int mno) { return 4 * ((size_t)(K_WORDS + 1) * K + (size_t)mno); }
    EVAL_HD static constexpr size_t slot_bytes(int K, int staged_) { return EVAL_PAIR_BYTES * (size_t)eval_odd(staged_) + 4 * (size_t)K; }
    EVAL_HD constexpr size_t bytes() const { return fixed_bytes(K, mno) + (size_t)SC * slot_bytes(K, Fp); }     // (Fp | 1 == Fp)
};
// The slot chunk: as many slots as the LDS holds next to the per-world words, spread evenly over the chunks of mno.  false: the per-world words
// and one slot do not fit: 40 K + 4 mno + 8 (F | 1) + 4 K > 61440.  At (mno 256, t_end 200, K 176) a chunk is 22 slots.
inline bool worlds_geometry(int mno, int K, int metric, int t_end, int* SC) {
    if (mno < 1 || K < 1 || t_end < 1) return false;
    const size_t fixed = WorldsLds::fixed_bytes(K, mno), per = WorldsLds::slot_bytes(K, SelLds::staged(metric, t_end));
    if (fixed + per > (size_t)EVAL_LDS_BYTES) return false;
    const size_t fit = ((size_t)EVAL_LDS_BYTES - fixed) / per;
    const int sc = (int)((size_t)mno < fit ? (size_t)mno : fit);
    *SC = eval_chunks(mno, eval_chunks(mno, sc));
    return true;
}
