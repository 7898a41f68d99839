"""Numpy statement of the ranking contract (include/desire_hip.h: desire_rank_samples / desire_ranked_errors) and the synthetic inputs
its tests share.  Agent a = scene * mno + slot, row r = (scene * K + k) * mno + slot."""
import numpy as np


def rank_order(score, d):                        # score [n,K,mno] -> [A,K] int32
    s = np.asarray(score, np.float32).reshape(d.n_scenes, d.K, d.mno).transpose(0, 2, 1).reshape(d.A, d.K)
    nan = np.isnan(s); key = np.where(nan, -np.inf, s).astype(np.float64)
    k = np.broadcast_to(np.arange(d.K), s.shape)
    return np.lexsort((k, -key, nan), axis=-1).astype(np.int32)


def ranked_errors(Y, fut, order, n_top, horizons, ux, uy, d):   # Y [R,T,2]; fut [n,T,mno,3] loader layout
    Yk = Y.reshape(d.n_scenes, d.K, d.mno, d.T_pred, 2).astype(np.float32); f = np.asarray(fut, np.float32)
    gx = (f[..., 1] * np.float32(d.sx)).transpose(0, 2, 1); gy = (f[..., 2] * np.float32(d.sy)).transpose(0, 2, 1)
    dx = (Yk[..., 0] - gx[:, None]) * np.float32(ux); dy = (Yk[..., 1] - gy[:, None]) * np.float32(uy)
    e = np.sqrt(dx * dx + dy * dy).astype(np.float32).transpose(0, 2, 1, 3).reshape(d.A, d.K, d.T_pred)
    pr = (f[..., 0] != 0).transpose(0, 2, 1).reshape(d.A, d.T_pred)
    out = np.zeros((d.A, len(horizons), 4), np.float32)
    for a in range(d.A):
        for hi, h in enumerate(horizons):
            idx = np.nonzero(pr[a, :h])[0]
            if idx.size == 0: continue
            ade = np.array([sum((e[a, k, t] for t in idx), np.float32(0)) / np.float32(idx.size) for k in range(d.K)], np.float32)
            fde = e[a, :, idx[-1]]; top = order[a, :n_top]
            out[a, hi] = (ade[top[0]], fde[top[0]], ade[top].min(), fde[top].min())
    return out


def planted_scores(d, seed):
    """[n, K, mno] fp32: random normal, plus -- where the shape has room -- a tie, a wholly tied agent, all-zero agents, NaN, +-inf, +-0."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((d.n_scenes, d.K, d.mno)).astype(np.float32)
    m, K = d.mno, d.K
    if K >= 3:
        s[0, 2, 0] = s[0, 0, 0]                                  # a tie: the lower k first
        s[-1, 0, m - 1] = np.nan                                 # a NaN at k = 0: last
    if m >= 2:
        s[0, :, 1] = 0.25                                        # a wholly tied agent: identity
        s[-1, :, 0] = 0.0                                        # all-zero agents (an absent slot under DESIRE_FLAG_COMPACT_IOC): identity
    if m >= 4:
        s[0, :, 3] = 0.0
        s[-1, :, 2] = np.nan                                     # all NaN: identity
    if m >= 8 and K >= 3:
        s[0, 1, 4] = np.inf; s[0, K - 1, 4] = -np.inf; s[0, 0, 4] = np.nan      # +inf first, -inf before the NaN
        s[0, 0, 5] = -0.0; s[0, 1, 5] = 0.0; s[0, 2, 5] = -0.0                  # +-0 tie: 0, 1, 2 keep their order
        s[0, 3:, 5] = -np.abs(s[0, 3:, 5]) - 1.0
        s[0, :, 6] = np.where(np.arange(K) % 2 == 0, np.nan, s[0, :, 6])        # several NaNs: among themselves by lower k
    return s
