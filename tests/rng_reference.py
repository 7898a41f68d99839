"""numpy restatement of desire_amd/csrc/philox.h: Philox4x32-10, the uniform map, Box-Muller (in float64, on the same bits) and the counter packing
that include/desire_hip.h states.  The integer stream is held bit-exact against it (tests/test_rng_cpu.py on the host, tests/test_gpu_rng.py on the
device); the fp32 normals of the library are held within 1e-5 of these float64 ones."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
MAX_L, MAX_SLOT, MAX_K = 4096, 512, 8192

# the published known answers of Philox4x32-10 (Random123's kat_vectors): (counter, key, output)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (broadcast against each other) -> [..., 4] uint32."""
    c = np.asarray(ctr, np.uint64) & MASK
    k = np.asarray(key, np.uint64) & MASK
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def uniform(x):
    """u = ((x >> 9) + 0.5) * 2^-23: 24 significant bits (exact in fp32), never 0 or 1."""
    return ((np.asarray(x, np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(bits):
    """[..., 4] uint32 -> [..., 4] float64: Box-Muller on (x0, x1) and (x2, x3); the pair's normals are r cos(theta), r sin(theta)."""
    u = uniform(bits)
    out = np.empty(u.shape, np.float64)
    for p in (0, 1):
        r, th = np.sqrt(-2.0 * np.log(u[..., 2 * p])), 2.0 * np.pi * u[..., 2 * p + 1]
        out[..., 2 * p], out[..., 2 * p + 1] = r * np.cos(th), r * np.sin(th)
    return out


def seed_key(seed):
    return np.array([seed & MASK, (seed >> 32) & MASK], np.uint64)


def eps_counter(draw, window, k, slot, l):
    """The four counter words of latent l (any l of the block) of sample k of (global window, global slot) in draw `draw`."""
    draw, window, k, slot, l = np.broadcast_arrays(*(np.asarray(v, np.uint64) for v in (draw, window, k, slot, l)))
    c0 = (l >> np.uint64(2)) | (slot << np.uint64(10)) | (k << np.uint64(19))
    return np.stack([c0 & MASK, window & MASK, draw & MASK, np.zeros_like(c0)], -1).astype(np.uint32)


def fill_counter(stream_id, block):
    block = np.asarray(block, np.uint64)
    return np.stack([block & MASK, block >> np.uint64(32), np.full_like(block, stream_id & MASK), np.ones_like(block)], -1).astype(np.uint32)


def fill_bits(seed, stream_id, first, n):
    """Elements first .. first + n of the fill stream (seed, stream_id): uint32 [n]."""
    b0, b1 = first >> 2, (first + n + 3) >> 2
    x = philox4x32_10(fill_counter(stream_id, np.arange(b0, b1, dtype=np.uint64)), seed_key(seed)).reshape(-1)
    return x[first - 4 * b0: first - 4 * b0 + n]


def fill_normals(seed, stream_id, first, n):
    """The same elements as float64 normals."""
    b0, b1 = first >> 2, (first + n + 3) >> 2
    x = philox4x32_10(fill_counter(stream_id, np.arange(b0, b1, dtype=np.uint64)), seed_key(seed))
    return normals(x).reshape(-1)[first - 4 * b0: first - 4 * b0 + n]


def latent_eps(seed, draw, n_scenes, K, mno, L, scene_base=0, slot_base=0):
    """float64 [n_scenes, K, mno, L]: the eps of a NULL-eps call (row r = (scene * K + k) * mno + slot)."""
    assert L % 4 == 0 and L <= MAX_L and slot_base + mno <= MAX_SLOT and K < MAX_K
    sc, k, sl, b = np.meshgrid(np.arange(n_scenes), np.arange(K), np.arange(mno), np.arange(L // 4), indexing="ij")
    c = eps_counter(draw, (scene_base + sc) & MASK, k, slot_base + sl, 4 * b)
    return normals(philox4x32_10(c, seed_key(seed))).reshape(n_scenes, K, mno, L)


def kolmogorov_distance(x):
    """sup |F_n - Phi| of a sample against the standard normal."""
    from math import erf, sqrt
    x = np.sort(np.asarray(x, np.float64))
    n = x.size
    cdf = 0.5 * (1.0 + np.frompyfunc(lambda v: erf(v / sqrt(2.0)), 1, 1)(x).astype(np.float64))
    i = np.arange(n, dtype=np.float64)
    return float(max(np.abs(cdf - i / n).max(), np.abs((i + 1) / n - cdf).max()))


# test 1 of tests/test_gpu_rng.py: the seed (and fill stream) whose 2^20 normals this restatement alone holds inside all three bounds
# (tests/test_rng_cpu.py: test_the_fixed_seed_of_the_stream_test_passes_on_the_restatement)
STREAM_SEED, STREAM_ID, STREAM_N = 20240, 7, 1 << 20


def moment_bounds(n):
    """(|mean|, |var - 1|, Kolmogorov distance) bounds at sample size n: five standard errors of the mean and of the variance of a normal sample, and
    the 1 % critical value of the one-sample Kolmogorov-Smirnov statistic."""
    return 5.0 / np.sqrt(n), 5.0 * np.sqrt(2.0 / n), 1.63 / np.sqrt(n)
