// philox_rng.h -- the generator behind the device-side reset sampler (physics.hip sample_init, apply_init, duckie_step,
// sampler_next_map): Philox4x32-10, the draw functions on top of it, and the counter layout of its streams.  Plain C++ without a HIP
// header: under hipcc every function is __host__ __device__, and a host compiler sees ordinary inline functions, so a host program can
// include it (tests/test_reset_sampler_model_host.py holds it to tests/reset_sampler_model.py word for word with g++ -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DT_RNG_FN __host__ __device__ inline
#else
#define DT_RNG_FN inline
#endif

// Counter layout of one env's streams.  All share the key (seed lo, seed hi ^ hash(env)) and the words ctr[2] = episode, ctr[3] = env;
// ctr[0] counts the blocks of a stream and carries into ctr[1], which names the stream:
//   reset stream      ctr[1] = 0                          ctr[0] = 0, 1, 2, ...  (49 words of draws + 6 per spawn attempt: < 2^14 blocks)
//   map stream        ctr[1] = DT_RNG_TAG_MAP             ctr[0] = 0             (one word)
//   object streams    ctr[1] = DT_RNG_TAG_OBJECT + slot   ctr[0] = the event: DT_OBJ_EVENT_WALK(step_count) for a finish_walk (5 words:
//                                                         2 blocks), or DT_OBJ_EVENT_CREATE for the creation (a domain-randomised
//                                                         DuckieObj: 6 words, 2 blocks; a DuckiebotObj: 16 words, 4 blocks)
// No two of these share a block (tests/test_reset_sampler_model_host.py::test_counter_blocks_are_disjoint enumerates them):
// DT_OBJ_EVENT_CREATE leaves 256 blocks to the end of its row, so a creation stream never carries into ctr[1], and a walk's event is
// twice its step_count (a positive int32), so walks at consecutive steps keep their second blocks apart and stay below the creation's.
// They stood at 0xFFFFFFFF and at step_count itself first: every block of a creation after its first then lay in the row of slot + 1, at
// that slot's walk events 0, 1 and 2, and the fifth word of a walk was the first of the next step's.
#define DT_RNG_TAG_OBJECT 0x4F424A00u
#define DT_RNG_TAG_MAP 0x4D415000u
#define DT_OBJ_EVENT_CREATE 0xFFFFFF00u
#define DT_OBJ_EVENT_WALK(step_count) (2u * (uint32_t)(step_count))

// Philox4x32-10 (Salmon et al. 2011): counter-based, so an env's draws for episode k depend only on
// (seed, env, k) -- reproducible regardless of which step the reset happens in or how envs are sharded.
struct Philox {
  uint32_t key[2], ctr[4], out[4];
  int left;
};
DT_RNG_FN void philox_round(uint32_t c[4], const uint32_t k[2]) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k[0], n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k[1];
  c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
}
DT_RNG_FN void philox_refill(Philox& g) {
  uint32_t c[4] = {g.ctr[0], g.ctr[1], g.ctr[2], g.ctr[3]}, k[2] = {g.key[0], g.key[1]};
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k);
    k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
  }
  for (int i = 0; i < 4; ++i) g.out[i] = c[i];
  g.left = 4;
  if (++g.ctr[0] == 0) ++g.ctr[1];
}
DT_RNG_FN Philox philox_init(uint64_t seed, uint32_t env, uint32_t episode) {
  Philox g;
  g.key[0] = (uint32_t)seed; g.key[1] = (uint32_t)(seed >> 32) ^ (env * 0x9E3779B1u + 0x7F4A7C15u);
  g.ctr[0] = 0; g.ctr[1] = 0; g.ctr[2] = episode; g.ctr[3] = env;
  g.left = 0;
  return g;
}
DT_RNG_FN uint32_t rng_u32(Philox& g) {
  if (g.left == 0) philox_refill(g);
  return g.out[--g.left];
}
DT_RNG_FN double rng_double(Philox& g) {     // [0,1) with 53 random bits (numpy's construction)
  const uint32_t a = rng_u32(g) >> 5, b = rng_u32(g) >> 6;
  return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
}
DT_RNG_FN double rng_uniform(Philox& g, double lo, double hi) { return lo + (hi - lo) * rng_double(g); }
DT_RNG_FN int rng_below(Philox& g, int n) { return (int)(((uint64_t)rng_u32(g) * (uint64_t)n) >> 32); }
DT_RNG_FN double rng_normal(Philox& g, double loc, double scale) {   // Box-Muller
  const double u1 = 1.0 - rng_double(g), u2 = rng_double(g);
  return loc + scale * sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}
// Stream of one dynamic object's domain-randomisation draws: same key as the env's reset stream, word 1 carries a tag + the dynamic
// slot, word 0 the event: DT_OBJ_EVENT_CREATE or DT_OBJ_EVENT_WALK (the layout: above).
DT_RNG_FN Philox philox_object(uint64_t seed, uint32_t env, uint32_t episode, uint32_t slot, uint32_t event) {
  Philox g = philox_init(seed, env, episode);
  g.ctr[0] = event; g.ctr[1] = DT_RNG_TAG_OBJECT + slot;
  return g;
}
