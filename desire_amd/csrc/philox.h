// philox.h -- the counter-based generator behind desire_set_rng / desire_rng_fill: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers:
// as easy as 1, 2, 3", SC'11), its map to uniforms and normals, and the packing of the counters (include/desire_hip.h states the packing: it is part
// of the contract).  A normal is a pure function of (seed, draw, global window, k, global slot, latent): it is computed where it is consumed and never stored.
// Host and device, no HIP include: tests/c_host/philox_driver.cpp and rollout_philox_driver.cpp compile it with g++ (tests/test_rng_cpu.py,
// tests/test_rollout_rng_cpu.py), tests/rng_reference.py and tests/rollout_reference.py restate it in numpy.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PHILOX_HD __host__ __device__ inline
#else
#define PHILOX_HD inline
#endif

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // Weyl constants of the key schedule
constexpr uint32_t PHILOX_EPS = 0u, PHILOX_FILL = 1u, PHILOX_ROLL = 2u;   // counter word c3: what the block is for
// limits of the latent packing below (desire_set_rng refuses dims outside them); the rollout packing adds T_pred <= PHILOX_MAX_T
constexpr int PHILOX_MAX_L = 4096, PHILOX_MAX_SLOT = 512, PHILOX_MAX_K = 8192, PHILOX_MAX_T = 2048;

struct Philox4 { uint32_t v[4]; };

PHILOX_HD Philox4 philox4x32_10(Philox4 c, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c.v[0], p1 = (uint64_t)PHILOX_M1 * c.v[2];
        const Philox4 n = {{(uint32_t)(p1 >> 32) ^ c.v[1] ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.v[3] ^ k1, (uint32_t)p0}};
        c = n;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    return c;
}

// u = ((x >> 9) + 0.5) * 2^-23: 24 significant bits, so every step is exact in fp32, and u is never 0 or 1
PHILOX_HD float philox_uniform(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// Box-Muller on the pairs (x0, x1) and (x2, x3): one block = four normals, |n| <= sqrt(48 ln 2) = 5.77
PHILOX_HD void philox_normal4(const Philox4& x, float out[4]) {
    for (int p = 0; p < 2; ++p) {
        const float r = sqrtf(-2.0f * logf(philox_uniform(x.v[2 * p])));
        const float th = 6.283185307179586f * philox_uniform(x.v[2 * p + 1]);
        out[2 * p] = r * cosf(th);
        out[2 * p + 1] = r * sinf(th);
    }
}

// ---- counters.  Latent eps: latent l of (draw, global window, k, global slot) is normal l & 3 of this block.
//   c0 = (l >> 2) | slot << 10 | k << 19     (L <= 4096, slot < 512, k < 8192)
//   c1 = global window (scene_base + scene, modulo 2^32) ; c2 = draw ; c3 = PHILOX_EPS
PHILOX_HD Philox4 philox_eps_counter(uint32_t draw, uint32_t window, uint32_t k, uint32_t slot, uint32_t l) {
    const Philox4 c = {{(l >> 2) | (slot << 10) | (k << 19), window, draw, PHILOX_EPS}};
    return c;
}
// Fill op (desire_rng_fill): element e of stream `stream_id` is word / normal e & 3 of block e >> 2.
//   c0, c1 = low, high word of the block index ; c2 = stream_id ; c3 = PHILOX_FILL
PHILOX_HD Philox4 philox_fill_counter(uint32_t stream_id, uint64_t block) {
    const Philox4 c = {{(uint32_t)block, (uint32_t)(block >> 32), stream_id, PHILOX_FILL}};
    return c;
}

// Head rollout (desire_rollout_samples): step t of sample k of (draw, global window, global slot) takes normals 2 (t & 1) and 2 (t & 1) + 1 of this block
// (the x and the y draw of the step), so one block serves two steps.
//   c0 = (t >> 1) | slot << 10 | k << 19     (T_pred <= 2048, slot < 512, k < 8192)
//   c1 = global window ; c2 = draw ; c3 = PHILOX_ROLL
PHILOX_HD Philox4 philox_roll_counter(uint32_t draw, uint32_t window, uint32_t k, uint32_t slot, uint32_t t) {
    const Philox4 c = {{(t >> 1) | (slot << 10) | (k << 19), window, draw, PHILOX_ROLL}};
    return c;
}

// the four eps of latents 4*(l >> 2) .. + 3 (key = the 64-bit seed as (lo, hi))
PHILOX_HD void philox_eps4(uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, uint32_t window, uint32_t k, uint32_t slot, uint32_t l, float out[4]) {
    philox_normal4(philox4x32_10(philox_eps_counter(draw, window, k, slot, l), seed_lo, seed_hi), out);
}
// the four rollout normals of steps 2*(t >> 1) and 2*(t >> 1) + 1: (x, y) of the even step, (x, y) of the odd one
PHILOX_HD void philox_roll4(uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, uint32_t window, uint32_t k, uint32_t slot, uint32_t t, float out[4]) {
    philox_normal4(philox4x32_10(philox_roll_counter(draw, window, k, slot, t), seed_lo, seed_hi), out);
}
