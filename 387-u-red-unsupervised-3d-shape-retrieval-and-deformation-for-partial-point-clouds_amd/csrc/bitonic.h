// bitonic.h — block-wide ascending bitonic sort of 64-bit keys in LDS, shared by occ.hip (the
// occlusion selections) and knn.h (the K > 32 nearest-neighbour selection). Include after
// ured_common.h (URED_DBG_CHECK records into the including file's word).
#pragma once

namespace ured {

// the waves of a block each at their own pace: orders a wave's LDS writes before its later reads
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ascending bitonic sort of keys[0, P2), P2 a power of two; every one of the block's T threads
// (T a multiple of 64) calls it with its thread index t.
// Thread t owns compare-exchange pair p = t (+ T ...) of each stage: elements i and i | j with
// i = p's bits above j shifted up by one. For j <= 64 the 64 pairs of a wave lie in one 128-element
// block of their own; a stage with j > 64 reads and writes across those blocks. So a block-wide
// barrier follows every stage whose own distance or whose successor's exceeds 64 (15 of the 66
// stages at 2048 keys); between two stages with j <= 64 the wave alone is synchronised.
template <int T>
__device__ void bitonic_sort_u64(unsigned long long* keys, int P2, int t) {
    static_assert(T % 64 == 0, "whole waves");
    __syncthreads();
    const int half = P2 >> 1;
    for (int k = 2; k <= P2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = t; p < half; p += T) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), q = i | j;
                URED_DBG_CHECK(q < P2);
                const unsigned long long a = keys[i], b = keys[q];
                if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[q] = a; }
            }
            const int next_j = j > 1 ? (j >> 1) : k;       // the next stage's distance (k: of 2k's first)
            if (j > 64 || next_j > 64) __syncthreads(); else wave_lds_sync();
        }
    }
    __syncthreads();
}

}  // namespace ured
