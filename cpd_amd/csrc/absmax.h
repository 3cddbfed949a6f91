// absmax.h -- the absmax block of the f16x2 range guard, device side (gfx950 only; wave = 64).
//
// An absmax block (include/cpd_hip.h) is CPD_ABSMAX_SLOTS words, CPD_ABSMAX_STRIDE words apart -- one per 128-byte line, because
// atomics on one line serialise. Each word holds the bits of a partial max |x| (non-negative floats order like their bits; NaN on
// top); the maximum of the tensor is the largest of them. Producers raise a block from their epilogues, consumers turn it into the
// power-of-two pre-scale of the fp16 split. Both rules live here and nowhere else.
#pragma once
#include "common.h"

// the slot this workgroup raises
__device__ __forceinline__ uint32_t *absmax_slot(uint32_t *block) { return block + (blockIdx.x & (CPD_ABSMAX_SLOTS - 1)) * CPD_ABSMAX_STRIDE; }

// vmax = bits of the largest |v| this lane has stored so far; `live`: the value counts (a row inside the tensor)
__device__ __forceinline__ void absmax_note(uint32_t &vmax, float v) {
    const uint32_t vb = __float_as_uint(v) & 0x7fffffffu;
    vmax = vb > vmax ? vb : vmax;
}
__device__ __forceinline__ void absmax_note(uint32_t &vmax, float v, bool live) {
    const uint32_t vb = __float_as_uint(v) & 0x7fffffffu;
    vmax = (live && vb > vmax) ? vb : vmax;
}

// Raise `block` (or NULL) to the lanes' vmax; every lane of the wave calls it. One (rarely issued) atomic per wave: the slot is read
// past the L1 first and raised only when this wave holds a larger value -- after the first workgroups almost nobody does.
__device__ __forceinline__ void absmax_raise(uint32_t *block, uint32_t vmax) {
    if (!block) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t t = (uint32_t)__shfl_xor((int)vmax, o);
        vmax = t > vmax ? t : vmax;
    }
    if ((threadIdx.x & 63) == 0) {
        uint32_t *slot = absmax_slot(block);
        if (vmax > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, vmax);
    }
}

// Power-of-two pre-scale of an input for the fp16 split: s = 2^(14 - floor(log2 max|in|)), inv = 1 / s (both exact); 1 without a block
__device__ __forceinline__ void in_pow2_scale(const uint32_t *absmax, float &s, float &inv) {
    s = 1.f; inv = 1.f;
    if (absmax) {
        uint32_t m = absmax[(threadIdx.x & (CPD_ABSMAX_SLOTS - 1)) * CPD_ABSMAX_STRIDE];     // lane i: slot i (mod CPD_ABSMAX_SLOTS)
#pragma unroll
        for (int o = CPD_ABSMAX_SLOTS / 2; o > 0; o >>= 1) {
            const uint32_t t = (uint32_t)__shfl_xor((int)m, o);
            m = t > m ? t : m;
        }
        m = (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
        const int e = (int)((m >> 23) & 0xffu);                // biased exponent of max |in|
        if (e != 0 && e != 255) {                              // zero / denormal / inf / nan maximum: left alone
            int se = 268 - e;                                  // 127 + 14 - (e - 127)
            se = se < 1 ? 1 : (se > 253 ? 253 : se);
            s = __uint_as_float((uint32_t)se << 23);
            inv = __uint_as_float((uint32_t)(254 - se) << 23);
        }
    }
}
