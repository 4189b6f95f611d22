// dropout_hash.h -- the counter-based keep-mask of the training kernels' dropout sites (formertrain.hip).  Integer operations only, host and device: a mask is a
// function of (seed, site, element index) and of nothing else (no launch geometry, no call order).  tests/former_model.py restates it with numpy integers.
//
//   m(x)   = the 32-bit finaliser  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
//   h      = m(lo32(seed) ^ (0x9e3779b9 * (site + 1)));  h = m(h ^ hi32(seed));  h = m(h ^ lo32(index));  h = m(h ^ hi32(index))
//   keep   = h >= floor(p * 2^32); a kept value is multiplied by the fp32 1 / (1 - p) the host computed
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VT_HASH_FN __host__ __device__ __forceinline__
#else
#define VT_HASH_FN static inline
#endif

#define VT_DROP_SITE_ATTN 0u  /* attention probabilities, index ((b H + h) T + i) T + j */
#define VT_DROP_SITE_1 1u     /* dropout1 (attention branch), index (b T + t) D + c */
#define VT_DROP_SITE_FF 2u    /* dropout (after the activation), index (b T + t) F + c */
#define VT_DROP_SITE_2 3u     /* dropout2 (feed-forward branch), index (b T + t) D + c */
/* the clip data set (clipdata.hip).  A clip's 64-bit key is hash(seed, KEY_LO, e) | hash(seed, KEY_HI, e) << 32 with e = epoch << 32 | global clip index; every
 * decision of the clip is hash(key, site, draw number): a function of (seed, epoch, clip index, draw number) and of nothing else.  A draw h maps to [lo, hi) by
 * multiply-shift, lo + ((uint64)h * (hi - lo) >> 32).  (Sites 100.. are the per-layer seeds of infill_training.layer_seed.) */
#define VT_CLIP_SITE_KEY_LO 16u
#define VT_CLIP_SITE_KEY_HI 17u
#define VT_CLIP_SITE_KID 18u        /* draw 0: the camera, [0, 4) */
#define VT_CLIP_SITE_DROP_LEN 19u   /* draw 0: [min_drop_len, max_drop_len + 1) */
#define VT_CLIP_SITE_START_FR 20u   /* draw 0: [start_fr_min, min(T - drop_len, start_fr_max)) */
#define VT_CLIP_SITE_AUG_START 21u  /* draw j < aug_num: the start of window j, [0, T - aug_num) */
#define VT_CLIP_SITE_NOISE 22u      /* draws 2 v, 2 v + 1: the two words of the normal value v = (j aug_num + frame in window) 3 + component */

VT_HASH_FN uint32_t vt_mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

VT_HASH_FN uint32_t vt_dropout_hash(uint64_t seed, uint32_t site, uint64_t index)
{
    uint32_t h = vt_mix32((uint32_t)seed ^ (0x9e3779b9u * (site + 1u)));
    h = vt_mix32(h ^ (uint32_t)(seed >> 32));
    h = vt_mix32(h ^ (uint32_t)index);
    h = vt_mix32(h ^ (uint32_t)(index >> 32));
    return h;
}
