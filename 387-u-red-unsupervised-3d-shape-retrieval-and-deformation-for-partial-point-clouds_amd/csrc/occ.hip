// occ.hip — partial (occluded) target clouds: the reference's dataset/gen_occ_point.py (ball,
// random, slice and part occlusion), the centring of partnet_dataset.py:60-62 and the optional
// rotation of partnet_dataset.py:73-78 (train_utils/random_rot.py) as ONE launch, one workgroup
// per sample, everything in LDS. No global atomics, no host sync, no allocation, no device state.
//
// N points in, K = N / 2 out (the reference asserts N = 2048, K = 1024), 16 <= N <= 4096.
//
// Random words.  word(seed, step, sample, stream, ctr) is output word 0 of Philox-4x32-10
// (Salmon et al., SC'11: multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 /
// 0xBB67AE85 added before rounds 2..10) with
//     key     = (seed & 0xffffffff, seed >> 32)
//     counter = ((stream << 16) | ctr, sample, step & 0xffffffff, step >> 32)     ctr < 65536
// and one round being  (c0, c1, c2, c3) <- (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1,
// lo(M0*c0)).  A uniform float of a word r is (r >> 8) * 2^-24, a uniform index in [0, n) is
// floor(r * n / 2^32).  Streams:
//     0  per-point keys of the random selections       ctr = point index
//     1  per-point keys of the ball centres            ctr = point index
//     2  the plan's scalars                            ctr = 0 mode, 1 ncenter, 2 slice centre,
//                                                      3..5 direction, 6 probe, 7..9 angles
//
// Plan (per sample; drawn in full whatever the mode, or given by the caller):
//   plan_i int32[12]: mode (u < 0.3f ball 0, < 0.6f random 1, < 0.9f slice 2, else part 3),
//                     ncenter = 1 << index4 (1, 2, 4, 8), 8 centre indices (the points with the 8
//                     smallest stream-1 keys, in key order; the first ncenter are used), the slice
//                     centre index, the part-mode probe index
//   plan_f fp32[6]:   slice direction c / sqrtf((cx*cx + cy*cy) + cz*cz), c = 1e-3f + u * (1.0f -
//                     1e-3f); three angles in degrees, -10.0f + 20.0f * u
//
// Selection is always "ranks [r0, r0 + K) of the ascending 64-bit keys (hi << 32) | point index"
// (unique keys, ties to the lower index) by a bitonic sort of the power-of-two padded array; hi is
// the bit pattern of a non-negative fp32 or a random word, ineligible points get the all-ones key.
//   random  hi = stream-0 word, every point eligible, r0 = 0
//   ball    for each used centre c the cancel = K / ncenter nearest points (itself included) by
//           (d, index), d = ((dx*dx) + (dy*dy)) + (dz*dz) in fp32, dx = x[i] - x[c], are cancelled;
//           then the survivors (at least K) with hi = stream-0 word, r0 = 0
//   slice   hi = bits of t = |((dx*nx) + (dy*ny)) + (dz*nz)|, dx = x[i] - x[centre]; r0 = K - 1:
//           ranks K-1 .. 2K-2 (the reference's dis_idx[nofp//2-1:-1]: the nearer half less one is
//           dropped, and the farthest point; for odd N the two farthest)
//   part    survivors sem[i] != sem[probe]; more than K of them: as the ball trim; else as random
// Outputs are in ascending point index. occ_mean is accumulated in fp64 (each thread its run of
// points in order, then a fixed tree over the threads); point_occ = R (x - mean) is evaluated in
// fp64 and rounded once, R = Rx Ry Rz of random_rot.py from the plan's angles (identity unless
// `rotate`).
#include <hip/hip_runtime.h>
#define URED_DBG_FILE 11
#include "ured_common.h"
#include "bitonic.h"
#include "../../include/ured_hip.h"

namespace {

constexpr int OC_T = 1024;
constexpr int OC_MAXN = 4096;
constexpr int OC_MINN = 16;
constexpr int OC_PI = URED_OCC_PLAN_I;
constexpr int OC_PF = URED_OCC_PLAN_F;
typedef unsigned long long u64;
typedef unsigned int u32;

__device__ __forceinline__ u32 occ_word(u64 seed, u64 step, u32 sample, u32 stream, u32 ctr) {
    u32 c0 = (stream << 16) | ctr, c1 = sample, c2 = (u32)step, c3 = (u32)(step >> 32);
    u32 k0 = (u32)seed, k1 = (u32)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0, n1 = (u32)p1, n2 = (u32)(p0 >> 32) ^ c3 ^ k1, n3 = (u32)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    }
    return c0;
}
__device__ __forceinline__ float occ_unif(u32 r) { return (float)(r >> 8) * 5.9604644775390625e-8f; }
__device__ __forceinline__ int occ_index(u32 r, int n) { return (int)(((u64)r * (u64)n) >> 32); }

// ascending bitonic sort of keys[0, P2), P2 a power of two; every thread of the block calls it
// (bitonic.h: the block-wide sort shared with the K-nearest-neighbour selection)
__device__ __forceinline__ void occ_sort(u64* keys, int P2, int t) { ured::bitonic_sort_u64<OC_T>(keys, P2, t); }

__global__ __launch_bounds__(OC_T) void occlude_kernel(const float* __restrict__ x, const long long* __restrict__ labels,
        const long long* __restrict__ sem, int N, u64 seed, u64 step, const int* __restrict__ modes,
        int mode_all, const int* __restrict__ plan_i_in, const float* __restrict__ plan_f_in, int rotate,
        long long* __restrict__ mask, float* __restrict__ ori, float* __restrict__ pocc,
        long long* __restrict__ labels_occ, long long* __restrict__ sem_occ, float* __restrict__ occ_mean,
        float* __restrict__ occ_rot, int* __restrict__ plan_i, float* __restrict__ plan_f) {
    __shared__ u64 keys[OC_MAXN];                    // sort keys; later the fp64 reduction scratch
    __shared__ unsigned char flag[OC_MAXN];          // alive (ball), then kept
    __shared__ int scan[OC_T];
    __shared__ u64 cmin[8];
    __shared__ int pi[OC_PI];
    __shared__ float pf[OC_PF];
    __shared__ int s_cnt;
    __shared__ double rot[9], mean[3];
    const int b = blockIdx.x, t = threadIdx.x;
    const int K = N / 2;
    int P2 = OC_MINN;
    while (P2 < N) P2 <<= 1;
    URED_DBG_CHECK(P2 <= OC_MAXN);
    const float* X = x + (size_t)b * N * 3;
    const long long* S = sem + (size_t)b * N;
    const long long* L = labels + (size_t)b * N;
    const u64 PAD = ~0ull;

    // ---- the plan ----
    if (plan_i_in) {                                  // given: indices clamped into the sample
        if (t < OC_PI) {
            const int v = plan_i_in[b * OC_PI + t];
            int lo = 0, hi = N - 1;
            if (t == 0) hi = 3;
            if (t == 1) { lo = 1; hi = 8; }
            URED_DBG_CHECK(v >= lo && v <= hi);
            pi[t] = min(max(v, lo), hi);
        }
        if (t < OC_PF) pf[t] = plan_f_in[b * OC_PF + t];
    } else {
        if (t < 8) cmin[t] = PAD;
        for (int i = t; i < N; i += OC_T) keys[i] = ((u64)occ_word(seed, step, b, 1, i) << 32) | (u32)i;
        __syncthreads();
        for (int r = 0; r < 8; ++r) {                 // the 8 smallest centre keys, in order
            const u64 prev = r ? cmin[r - 1] : 0;
            u64 m = PAD;
            for (int i = t; i < N; i += OC_T) {
                const u64 k = keys[i];
                if ((r == 0 || k > prev) && k < m) m = k;
            }
            for (int o = 32; o > 0; o >>= 1) {        // one LDS atomic per wave
                const u64 v = __shfl_xor(m, o);
                m = v < m ? v : m;
            }
            if ((t & 63) == 0 && m != PAD) atomicMin(&cmin[r], m);
            __syncthreads();
        }
        if (t < 8) {
            const int c = (int)(cmin[t] & 0xffffffffu);
            URED_DBG_CHECK(c >= 0 && c < N);
            pi[2 + t] = min(max(c, 0), N - 1);
        }
        if (t == 0) {
            const float u = occ_unif(occ_word(seed, step, b, 2, 0));
            int m = u < 0.3f ? 0 : u < 0.6f ? 1 : u < 0.9f ? 2 : 3;
            const int forced = modes ? modes[b] : mode_all;
            if (forced >= 0) {
                URED_DBG_CHECK(forced <= 3);
                m = min(forced, 3);
            }
            pi[0] = m;
            pi[1] = 1 << occ_index(occ_word(seed, step, b, 2, 1), 4);
            pi[10] = occ_index(occ_word(seed, step, b, 2, 2), N);
            pi[11] = occ_index(occ_word(seed, step, b, 2, 6), N);
            float c[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) c[a] = 1e-3f + occ_unif(occ_word(seed, step, b, 2, 3 + a)) * (1.0f - 1e-3f);
            const float nrm = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                pf[a] = c[a] / nrm;
                pf[3 + a] = -10.0f + 20.0f * occ_unif(occ_word(seed, step, b, 2, 7 + a));
            }
        }
    }
    __syncthreads();
    if (t < OC_PI) plan_i[b * OC_PI + t] = pi[t];
    if (t < OC_PF) plan_f[b * OC_PF + t] = pf[t];
    if (t == 0) {
        if (rotate) {
            const double d2r = 3.14159265358979323846 / 180.0;
            const double ax = (double)pf[3] * d2r, ay = (double)pf[4] * d2r, az = (double)pf[5] * d2r;
            const double cx = cos(ax), sx = sin(ax), cy = cos(ay), sy = sin(ay), cz = cos(az), sz = sin(az);
            // Rx = [1 0 0; 0 cx sx; 0 -sx cx], Ry = [cy 0 -sy; 0 1 0; sy 0 cy], Rz = [cz sz 0; -sz cz 0; 0 0 1]
            const double xy[9] = {cy, 0.0, -sy, sx * sy, cx, sx * cy, cx * sy, -sx, cx * cy};     // Rx Ry
            for (int r = 0; r < 3; ++r) {
                rot[3 * r + 0] = xy[3 * r] * cz - xy[3 * r + 1] * sz;
                rot[3 * r + 1] = xy[3 * r] * sz + xy[3 * r + 1] * cz;
                rot[3 * r + 2] = xy[3 * r + 2];
            }
        } else {
            for (int r = 0; r < 9; ++r) rot[r] = (r % 4 == 0) ? 1.0 : 0.0;
        }
    }

    // ---- the kept set: flag[i] = 1 for exactly K points ----
    int mode = pi[0];
    for (int i = t; i < N; i += OC_T) flag[i] = 1;
    __syncthreads();
    if (mode == 0) {                                  // ball: cancel around each centre
        const int nc = pi[1], cancel = K / nc;
        for (int c = 0; c < nc; ++c) {
            const int ci = pi[2 + c];
            const float cx = X[3 * ci], cy = X[3 * ci + 1], cz = X[3 * ci + 2];
            for (int i = t; i < P2; i += OC_T) {
                u64 k = PAD;
                if (i < N) {
                    const float dx = X[3 * i] - cx, dy = X[3 * i + 1] - cy, dz = X[3 * i + 2] - cz;
                    const float d = ((dx * dx) + (dy * dy)) + (dz * dz);
                    k = ((u64)__float_as_uint(d) << 32) | (u32)i;
                }
                keys[i] = k;
            }
            occ_sort(keys, P2, t);
            for (int j = t; j < cancel; j += OC_T) {
                const u32 i = (u32)(keys[j] & 0xffffffffu);
                URED_DBG_CHECK(i < (u32)N);
                if (i < (u32)N) flag[i] = 0;
            }
            __syncthreads();
        }
    } else if (mode == 3) {                           // part: drop the probe's semantic class
        if (t == 0) s_cnt = 0;
        __syncthreads();
        const long long s = S[pi[11]];
        int cnt = 0;
        for (int i = t; i < N; i += OC_T) {
            const int keep = S[i] != s;
            flag[i] = keep;
            cnt += keep;
        }
        if (cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        if (s_cnt <= K) {                             // the reference's else branch: plain random
            mode = 1;
            for (int i = t; i < N; i += OC_T) flag[i] = 1;
        }
        __syncthreads();
    }
    int r0 = 0;
    if (mode == 2) {                                  // slice: distance to the plane
        const int ci = pi[10];
        const float cx = X[3 * ci], cy = X[3 * ci + 1], cz = X[3 * ci + 2];
        const float nx = pf[0], ny = pf[1], nz = pf[2];
        for (int i = t; i < P2; i += OC_T) {
            u64 k = PAD;
            if (i < N) {
                const float dx = X[3 * i] - cx, dy = X[3 * i + 1] - cy, dz = X[3 * i + 2] - cz;
                const float d = fabsf(((dx * nx) + (dy * ny)) + (dz * nz));
                k = ((u64)__float_as_uint(d) << 32) | (u32)i;
            }
            keys[i] = k;
        }
        r0 = K - 1;
    } else {                                          // the eligible points by their stream-0 words
        for (int i = t; i < P2; i += OC_T)
            keys[i] = (i < N && flag[i]) ? (((u64)occ_word(seed, step, b, 0, i) << 32) | (u32)i) : PAD;
    }
    occ_sort(keys, P2, t);
    for (int i = t; i < N; i += OC_T) flag[i] = 0;
    __syncthreads();
    URED_DBG_CHECK(r0 + K <= N);
    for (int j = t; j < K; j += OC_T) {
        const u32 i = (u32)(keys[r0 + j] & 0xffffffffu);
        URED_DBG_CHECK(i < (u32)N);
        if (i < (u32)N) flag[i] = 1;
    }
    __syncthreads();

    // ---- ascending positions of the kept points, their fp64 sum ----
    const int per = (N + OC_T - 1) / OC_T, n0 = min(N, t * per), n1 = min(N, n0 + per);
    int cnt = 0;
    double s3[3] = {0.0, 0.0, 0.0};
    for (int n = n0; n < n1; ++n) {
        if (flag[n]) {
            ++cnt;
#pragma unroll
            for (int c = 0; c < 3; ++c) s3[c] += (double)X[3 * n + c];
        }
    }
    scan[t] = cnt;
    double* red = reinterpret_cast<double*>(keys);    // [3][OC_T] (24 KB of the 32)
#pragma unroll
    for (int c = 0; c < 3; ++c) red[c * OC_T + t] = s3[c];
    __syncthreads();
    for (int o = 1; o < OC_T; o <<= 1) {              // inclusive scan of the counts
        const int v = t >= o ? scan[t - o] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    for (int o = OC_T / 2; o > 0; o >>= 1) {          // fixed tree
        if (t < o) {
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c * OC_T + t] += red[c * OC_T + t + o];
        }
        __syncthreads();
    }
    if (t < 3) {
        mean[t] = red[t * OC_T] / (double)K;
        occ_mean[b * 3 + t] = (float)mean[t];
    }
    if (t < 9) occ_rot[b * 9 + t] = (float)rot[t];
    URED_DBG_CHECK(scan[OC_T - 1] == K);
    __syncthreads();
    int pos = scan[t] - cnt;
    for (int n = n0; n < n1; ++n) {
        if (!flag[n]) continue;
        URED_DBG_CHECK(pos >= 0 && pos < K);
        if (pos < K) {
            const size_t o = (size_t)b * K + pos;
            mask[o] = n;
            labels_occ[o] = L[n];
            sem_occ[o] = S[n];
            double d[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = X[3 * n + c];
                ori[o * 3 + c] = v;
                d[c] = (double)v - mean[c];
            }
#pragma unroll
            for (int r = 0; r < 3; ++r)
                pocc[o * 3 + r] = (float)((rot[3 * r] * d[0] + rot[3 * r + 1] * d[1]) + rot[3 * r + 2] * d[2]);
        }
        ++pos;
    }
}

}  // namespace

extern "C" int ured_occlude(const float* x, const long long* labels, const long long* sem, int B, int N,
                            unsigned long long seed, unsigned long long step, const int* modes,
                            int mode_all, const int* plan_i_in, const float* plan_f_in, int rotate, long long* mask,
                            float* ori_point_occ, float* point_occ, long long* labels_occ, long long* sem_occ,
                            float* occ_mean, float* occ_rot, int* plan_i, float* plan_f, void* stream) {
    ured::clear_error();
    URED_REQUIRE(B >= 0, "ured_occlude: negative size (B %d)", B);
    URED_REQUIRE(N >= OC_MINN && N <= OC_MAXN, "ured_occlude: N %d outside [%d, %d]", N, OC_MINN, OC_MAXN);
    URED_REQUIRE((plan_i_in == nullptr) == (plan_f_in == nullptr), "ured_occlude: plan_i_in and plan_f_in go together");
    URED_REQUIRE(mode_all >= -1 && mode_all <= 3, "ured_occlude: mode_all %d outside [-1, 3]", mode_all);
    URED_REQUIRE(!(plan_i_in && (modes || mode_all >= 0)),
                 "ured_occlude: a given plan carries its mode; modes must be null and mode_all -1");
    URED_REQUIRE(!(modes && mode_all >= 0), "ured_occlude: modes and mode_all exclude each other");
    if (B == 0) return 0;
    URED_REQUIRE((long long)B * N < (1LL << 31) / 3, "ured_occlude: too many points");
    URED_REQUIRE(x && labels && sem && mask && ori_point_occ && point_occ && labels_occ && sem_occ && occ_mean &&
                 occ_rot && plan_i && plan_f, "ured_occlude: null pointer");
    hipLaunchKernelGGL(occlude_kernel, dim3(B), dim3(OC_T), 0, (hipStream_t)stream, x, labels, sem, N, seed, step,
                       modes, mode_all, plan_i_in, plan_f_in, rotate, mask, ori_point_occ, point_occ, labels_occ, sem_occ,
                       occ_mean, occ_rot, plan_i, plan_f);
    return ured::launch_status("ured_occlude");
}

URED_DBG_ACCESSOR(ured_dbg_occ)
