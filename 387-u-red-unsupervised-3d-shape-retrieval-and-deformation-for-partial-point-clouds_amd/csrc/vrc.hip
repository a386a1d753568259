// vrc.hip — the kernels of VRCNet's self-attention encoder that are not GEMMs, for MI355X / gfx950
// (Density_aware_Chamfer_Distance/models/vrcnet.py:15-290): the attention core of SA_module, the two
// passes of SK_SA_module's branch selection, edge-preserved pooling and three-point unpooling with
// given weights. Activations are point-major [B*N][C] fp32. Plain pointers, the caller's stream, no
// allocation, no host sync, no device state, no float atomics; every limit is checked on the host
// before any device work. The file is built with -ffp-contract=off: a product and an add stay two
// roundings, and every sum below runs in the order its comment states.
//
// ured_vrc_sa_fwd. One wave per point n of P = [x1 | x2p | x3p] ([B*N][2 rel + mid]); the point's
//   u, h, w and neighbour rows live in the wave's slice of LDS:
//     u[i]  = max(x1[n][i], 0), i < rel;  u[rel + r k + j] = max(x2p[idx[n][j]][r], 0)
//     h[s]  = max(sum_i Wa[s][i] u[i], 0): lane l sums i = l, l + 64, .. ascending, then the 64 lane
//             sums meet in a butterfly (xor 32, 16, .., 1)
//     w[t]  = (sum_s Wb[t][s] h[s], s ascending) + bb[t], t < k ms, read as w[s][j] = w[s k + j]
//     o[c]  = max(sum_j w[c mod ms][j] x3p[idx[n][j]][c], 0), j ascending
//   An index outside [0, N) reads as a zero row. h [B*N][ms] and w [B*N][k ms] are written for the
//   backward; nothing of size k x mid or k x C is.
// ured_vrc_sa_bwd. Three launches.
//   point:   per point, G = go where o > 0 else 0 (written to gm); dw[s k + j] = sum over c = s, s + ms, ..
//            of G[c] x3p[idx[n][j]][c]; dh[s] = (sum_t Wb[t][s] dw[t], t ascending) where h[s] > 0 else 0;
//            dP[n][r] = (sum_s Wa[s][r] dh[s]) where x1[n][r] > 0 else 0, r < rel.
//   scatter: the scheme of group_bwd_kernel (csrc/group.hip). One wave per (32 points, 64 of the
//            rel + mid scattered columns) of a cloud scans the cloud's N k indices in order and adds,
//            for each entry (n, j) that names one of its points m, in ascending (n, j):
//            x2p column r:  sum_s Wa[s][rel + r k + j] dh[n][s] (s ascending), the total kept where
//            x2p[m][r] > 0; x3p column c: G[n][c] * w[n][(c mod ms) k + j]. Every element of
//            dP[:, rel:] is written once; a point no row names gets 0; an index outside [0, N)
//            takes no gradient.
//   wa:      dWa partials. One workgroup per `chunk` consecutive points; thread t owns columns
//            i = t, t + 256, .. and adds dh[n][s] * u[n][i] over the chunk's points in ascending
//            order; ws[chunk][s][i] is written, the caller sums the chunks (column sums, fixed order).
//   dWb = dw^T h and dbb = colsum(dw) are the caller's GEMM and column sum.
// ured_vrc_sk_mean_fwd / _bwd, ured_vrc_sk_mix_fwd / _bwd: see include/ured_hip.h.
// ured_vrc_pool_fwd / _bwd, ured_vrc_unpool_fwd / _bwd: see include/ured_hip.h.
// The decoder (EF_expansion of utils/model_utils.py:137-166, Folding of models/vrcnet.py:54-86):
// ured_vrc_ef_edge_fwd / _bwd  per-edge rows max((G +) centre[n] + neighbour[idx[n][j]], 0) from per-point
//   halves; the backward sums the centre half over j and scatters the neighbour half in the ordered
//   scheme of ured_vrc_sa_bwd.
// ured_vrc_ef_max_fwd / _bwd   the max over the k slots of conv3's rows, with the winning slot.
// ured_vrc_fold_fwd / _bwd     max(U[n] + T[s], 0) over the r grid points of every coarse point.
// Model's variational part (models/vrcnet.py:430-501):
// ured_vrc_latent_fwd / _bwd   softplus, the reparameterised samples of posterior and prior stacked as the
//   generator's [2B][Z] input, and the two KL terms in torch's kl_divergence form; one launch each way.
// ured_vrc_gauss_fwd / _bwd    compute_kernel's exp(-mean_d((x_i - y_j)^2) / Z) from direct differences, one
//   wave per pair; the backward sums over the other set's rows in ascending order.
#include <hip/hip_runtime.h>
#include <cstdint>
#define URED_DBG_FILE 18
#include "ured_common.h"
#include "../../include/ured_hip.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int VRC_T = 256;
constexpr int VRC_W = VRC_T / 64;                     // waves (points) of one attention workgroup
constexpr int VRC_KMAX = URED_VRC_KMAX, VRC_RELMAX = URED_VRC_RELMAX, VRC_MIDMAX = URED_VRC_MIDMAX;
constexpr int VRC_MSMAX = URED_VRC_MSMAX;
constexpr int VRC_LMAX = VRC_RELMAX * (VRC_KMAX + 1); // the longest u
constexpr int VRC_LQ = (VRC_LMAX + VRC_T - 1) / VRC_T; // columns of dWa one thread owns
constexpr int VRC_WB = 8;                             // points staged per step of the dWa kernel
constexpr int SC_P = 32, SC_C = 64;                   // points x channels of one scatter wave

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// rows of the cloud's neighbours in the [B*N] matrix, -1 for an index outside [0, N)
__device__ __forceinline__ void load_rows(const int* __restrict__ idx, size_t r, bool valid, int b, int N, int k, int ln,
                                          int* srow) {
    if (ln < k) {
        const int id = valid ? idx[r * k + ln] : -1;
        const int row = (id >= 0 && id < N) ? b * N + id : -1;  // B * N < 2^31 (host check)
        URED_DBG_CHECK(row < 0 || ((long long)row >= (long long)b * N && (long long)row < ((long long)b + 1) * N));
        srow[ln] = row;
    }
}

__global__ __launch_bounds__(VRC_T) void sa_fwd_kernel(const float* __restrict__ P, const int* __restrict__ idx,
                                                       const float* __restrict__ Wa, const float* __restrict__ Wb,
                                                       const float* __restrict__ bb, u32 BN, int N, int k, int rel, int mid,
                                                       int ms, float* __restrict__ o, float* __restrict__ h_out,
                                                       float* __restrict__ w_out) {
    __shared__ float su[VRC_W][VRC_LMAX];
    __shared__ float sh[VRC_W][VRC_MSMAX];
    __shared__ float sw[VRC_W][VRC_KMAX * VRC_MSMAX];
    __shared__ int srow[VRC_W][VRC_KMAX];
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * VRC_W + wv;
    const bool valid = r < BN;                        // no early exit: every wave meets every barrier
    const int b = valid ? (int)(r / (u32)N) : 0;
    const int ldp = 2 * rel + mid, L = rel * (k + 1), T = k * ms;
    load_rows(idx, r, valid, b, N, k, ln, srow[wv]);
    __syncthreads();
    for (int i = ln; i < L; i += 64) {
        float v = 0.f;
        if (i < rel) {
            if (valid) v = P[r * ldp + i];
        } else {
            const int q = i - rel, rr = q / k, j = q - rr * k;
            const int row = srow[wv][j];
            URED_DBG_CHECK(rr < rel && j < k && (row < 0 || (u32)row < BN));
            if (row >= 0) v = P[(size_t)row * ldp + rel + rr];
        }
        su[wv][i] = fmaxf(v, 0.f);
    }
    __syncthreads();
    for (int s = 0; s < ms; ++s) {
        float part = 0.f;
        for (int i = ln; i < L; i += 64) {
            const float pr = Wa[(size_t)s * L + i] * su[wv][i];
            part += pr;
        }
        part = wave_sum(part);
        if (ln == 0) sh[wv][s] = fmaxf(part, 0.f);
    }
    __syncthreads();
    for (int t = ln; t < T; t += 64) {
        float acc = 0.f;
        for (int s = 0; s < ms; ++s) {
            const float pr = Wb[(size_t)t * ms + s] * sh[wv][s];
            acc += pr;
        }
        acc += bb[t];
        sw[wv][t] = acc;
        URED_DBG_CHECK(t < VRC_KMAX * VRC_MSMAX && (!valid || r * T + t < (size_t)BN * T));
        if (valid) w_out[r * T + t] = acc;
    }
    URED_DBG_CHECK(!(ln < ms && valid) || r * ms + ln < (size_t)BN * ms);
    if (ln < ms && valid) h_out[r * ms + ln] = sh[wv][ln];
    __syncthreads();
    for (int c = ln; c < mid; c += 64) {
        const int s = c % ms;
        float acc = 0.f;
        for (int j = 0; j < k; ++j) {
            const int row = srow[wv][j];
            URED_DBG_CHECK(row < 0 || (u32)row < BN);
            const float x3 = row >= 0 ? P[(size_t)row * ldp + 2 * rel + c] : 0.f;
            const float pr = sw[wv][s * k + j] * x3;
            acc += pr;
        }
        if (valid) {
            URED_DBG_CHECK(r * mid + c < (size_t)BN * mid);
            o[r * mid + c] = fmaxf(acc, 0.f);
        }
    }
}

__global__ __launch_bounds__(VRC_T) void sa_bwd_point_kernel(const float* __restrict__ go, const float* __restrict__ o,
                                                             const float* __restrict__ P, const int* __restrict__ idx,
                                                             const float* __restrict__ Wa, const float* __restrict__ Wb,
                                                             const float* __restrict__ h, u32 BN, int N, int k, int rel,
                                                             int mid, int ms, float* __restrict__ gm, float* __restrict__ dw,
                                                             float* __restrict__ dh, float* __restrict__ dP) {
    __shared__ float sg[VRC_W][VRC_MIDMAX];
    __shared__ float sdw[VRC_W][VRC_KMAX * VRC_MSMAX];
    __shared__ float sdh[VRC_W][VRC_MSMAX];
    __shared__ int srow[VRC_W][VRC_KMAX];
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * VRC_W + wv;
    const bool valid = r < BN;
    const int b = valid ? (int)(r / (u32)N) : 0;
    const int ldp = 2 * rel + mid, L = rel * (k + 1), T = k * ms;
    load_rows(idx, r, valid, b, N, k, ln, srow[wv]);
    for (int c = ln; c < mid; c += 64) {
        float g = 0.f;
        if (valid) {
            g = o[r * mid + c] > 0.f ? go[r * mid + c] : 0.f;
            gm[r * mid + c] = g;
        }
        sg[wv][c] = g;
    }
    __syncthreads();
    for (int t = ln; t < T; t += 64) {
        const int s = t / k, j = t - s * k;
        const int row = srow[wv][j];
        float acc = 0.f;
        URED_DBG_CHECK(s < ms && j < k && (row < 0 || (u32)row < BN));
        if (row >= 0) {
            const float* x3 = P + (size_t)row * ldp + 2 * rel;
            for (int c = s; c < mid; c += ms) {
                const float pr = sg[wv][c] * x3[c];
                acc += pr;
            }
        }
        sdw[wv][t] = acc;
        URED_DBG_CHECK(t < VRC_KMAX * VRC_MSMAX && (!valid || r * T + t < (size_t)BN * T));
        if (valid) dw[r * T + t] = acc;
    }
    __syncthreads();
    if (ln < ms) {
        float acc = 0.f;
        for (int t = 0; t < T; ++t) {
            const float pr = Wb[(size_t)t * ms + ln] * sdw[wv][t];
            acc += pr;
        }
        const float v = (valid && h[r * ms + ln] > 0.f) ? acc : 0.f;
        sdh[wv][ln] = v;
        URED_DBG_CHECK(!valid || r * ms + ln < (size_t)BN * ms);
        if (valid) dh[r * ms + ln] = v;
    }
    __syncthreads();
    if (ln < rel && valid) {
        float acc = 0.f;
        for (int s = 0; s < ms; ++s) {
            const float pr = Wa[(size_t)s * L + ln] * sdh[wv][s];
            acc += pr;
        }
        URED_DBG_CHECK(r * ldp + ln < (size_t)BN * ldp);
        dP[r * ldp + ln] = P[r * ldp + ln] > 0.f ? acc : 0.f;
    }
}

// The ordered scatter of group_bwd_kernel: the wave scans the E indices of I in order, 64 at a time,
// picks the entries that land in its SC_P points [j0, j0 + SC_P) (a ballot, walked from its lowest
// bit) and adds f(entry) to the point's accumulator. Column ln of acc belongs to lane ln alone.
template <class F>
__device__ __forceinline__ void scan_add(const int* __restrict__ I, int E, int j0, int ln, float* acc, F f) {
    for (int e0 = 0; e0 < E; e0 += 64) {
        const int e = e0 + ln;
        const int id = e < E ? I[e] : -1;
        const int p = id - j0;                        // id = -1 and j0 >= 0: never in [0, SC_P)
        u64 mask = __ballot(id >= 0 && (u32)p < (u32)SC_P);
        while (mask) {
            const int l = (int)__builtin_ctzll(mask);
            mask &= mask - 1;
            const int pp = __shfl(p, l);
            URED_DBG_CHECK(pp >= 0 && pp < SC_P && e0 + l < E);
            if (pp >= 0 && pp < SC_P) acc[pp * SC_C + ln] += f(e0 + l);
        }
    }
}

__global__ __launch_bounds__(64) void sa_bwd_scatter_kernel(const float* __restrict__ gm, const float* __restrict__ w,
                                                            const float* __restrict__ dh, const float* __restrict__ P,
                                                            const int* __restrict__ idx, const float* __restrict__ Wa, int N,
                                                            int k, int rel, int mid, int ms, int tiles_n,
                                                            float* __restrict__ dP) {
    __shared__ float acc[SC_P * SC_C];
    const int ln = threadIdx.x, b = blockIdx.y;
    const int tn = blockIdx.x % tiles_n, tc = blockIdx.x / tiles_n;
    const int j0 = tn * SC_P, cc = tc * SC_C + ln;
    const int ldp = 2 * rel + mid, L = rel * (k + 1), T = k * ms, E = N * k;   // N * k < 2^31 (host check)
    const bool cin = cc < rel + mid, is2 = cc < rel;
    const int c3 = cc - rel;                          // the x3p channel of a lane past the x2p columns
    const int s3 = cin && !is2 ? c3 % ms : 0;
    const size_t base = (size_t)b * N;
#pragma unroll
    for (int p = 0; p < SC_P; ++p) acc[p * SC_C + ln] = 0.f;
    scan_add(idx + base * k, E, j0, ln, acc, [&](int e) -> float {
        if (!cin) return 0.f;
        const int n = e / k, j = e - n * k;
        const size_t rn = base + n;
        URED_DBG_CHECK(n < N && (is2 ? rel + cc * k + j < L : s3 * k + j < T));
        if (is2) {
            float t = 0.f;
            for (int s = 0; s < ms; ++s) {
                const float pr = Wa[(size_t)s * L + rel + cc * k + j] * dh[rn * ms + s];
                t += pr;
            }
            return t;
        }
        return gm[rn * mid + c3] * w[rn * T + s3 * k + j];
    });
    if (!cin) return;
    for (int p = 0; p < SC_P; ++p) {
        const int m = j0 + p;
        if (m >= N) break;
        const size_t at = (base + m) * ldp + rel + cc;
        URED_DBG_CHECK(rel + cc < ldp && at < (size_t)gridDim.y * N * ldp);
        float v = acc[p * SC_C + ln];
        if (is2 && !(P[at] > 0.f)) v = 0.f;
        dP[at] = v;
    }
}

__global__ __launch_bounds__(VRC_T) void sa_bwd_wa_kernel(const float* __restrict__ dh, const float* __restrict__ P,
                                                          const int* __restrict__ idx, u32 BN, int N, int k, int rel, int mid,
                                                          int ms, int chunk, float* __restrict__ ws) {
    __shared__ int srow[VRC_WB][VRC_KMAX];
    __shared__ float sdh[VRC_WB][VRC_MSMAX];
    const int t = threadIdx.x;
    const int ldp = 2 * rel + mid, L = rel * (k + 1);
    const size_t p0 = (size_t)blockIdx.x * chunk;
    const size_t p1 = p0 + chunk < BN ? p0 + chunk : BN;
    float acc[VRC_LQ][VRC_MSMAX];
#pragma unroll
    for (int q = 0; q < VRC_LQ; ++q)
#pragma unroll
        for (int s = 0; s < VRC_MSMAX; ++s) acc[q][s] = 0.f;
    for (size_t pb = p0; pb < p1; pb += VRC_WB) {     // the same trip count for every thread
        __syncthreads();
        for (int e = t; e < VRC_WB * VRC_KMAX; e += VRC_T) {
            const int pi = e / VRC_KMAX, j = e - pi * VRC_KMAX;
            const size_t r = pb + pi;
            int row = -1;
            if (r < p1 && j < k) {
                const int id = idx[r * k + j];
                const int bq = (int)(r / (u32)N);
                if (id >= 0 && id < N) row = bq * N + id;
            }
            srow[pi][j] = row;
        }
        for (int e = t; e < VRC_WB * VRC_MSMAX; e += VRC_T) {
            const int pi = e / VRC_MSMAX, s = e - pi * VRC_MSMAX;
            const size_t r = pb + pi;
            sdh[pi][s] = (r < p1 && s < ms) ? dh[r * ms + s] : 0.f;
        }
        __syncthreads();
        for (int pi = 0; pi < VRC_WB; ++pi) {
            const size_t r = pb + pi;
            if (r >= p1) break;                       // uniform over the workgroup
#pragma unroll
            for (int q = 0; q < VRC_LQ; ++q) {
                const int i = t + q * VRC_T;
                if (i < L) {
                    float v = 0.f;
                    if (i < rel) {
                        v = P[r * ldp + i];
                    } else {
                        const int qq = i - rel, rr = qq / k, j = qq - rr * k;
                        const int row = srow[pi][j];
                        URED_DBG_CHECK(rr < rel && j < k && (row < 0 || (u32)row < BN));
                        if (row >= 0) v = P[(size_t)row * ldp + rel + rr];
                    }
                    v = fmaxf(v, 0.f);
#pragma unroll
                    for (int s = 0; s < VRC_MSMAX; ++s) {
                        const float pr = sdh[pi][s] * v;      // rows s >= ms of sdh are 0
                        acc[q][s] += pr;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < VRC_LQ; ++q) {
        const int i = t + q * VRC_T;
        if (i < L) {
#pragma unroll
            for (int s = 0; s < VRC_MSMAX; ++s)
                if (s < ms) {
                    URED_DBG_CHECK(((size_t)blockIdx.x * ms + s) * L + i < (size_t)gridDim.x * ms * L);
                    ws[((size_t)blockIdx.x * ms + s) * L + i] = acc[q][s];
                }
        }
    }
}

// ---------------- SK selection ----------------

struct Branches {
    const float* y[URED_VRC_MMAX];
};
struct BranchesOut {
    float* y[URED_VRC_MMAX];
};

constexpr int SK_G = VRC_T / 64;                      // row groups of one reduction workgroup

// s[b][c] = (sum over n of (f_0 + f_1 + ..)[b][n][c]) / N, f_i = max(y_i, 0): row group g sums the rows
// n = g, g + SK_G, .. ascending, the SK_G sums are added in ascending g, then the division.
__global__ __launch_bounds__(VRC_T) void sk_mean_fwd_kernel(Branches Y, int m, int N, int C, float* __restrict__ s_out) {
    __shared__ float part[SK_G][64];
    const int g = threadIdx.x >> 6, cl = threadIdx.x & 63;
    const int c = blockIdx.x * 64 + cl, b = blockIdx.y;
    float acc = 0.f;
    if (c < C) {
        for (int n = g; n < N; n += SK_G) {
            const size_t at = ((size_t)b * N + n) * C + c;
            float U = fmaxf(Y.y[0][at], 0.f);
            for (int i = 1; i < m; ++i) U += fmaxf(Y.y[i][at], 0.f);
            acc += U;
        }
    }
    part[g][cl] = acc;
    __syncthreads();
    if (g == 0 && c < C) {
        float t = part[0][cl];
#pragma unroll
        for (int q = 1; q < SK_G; ++q) t += part[q][cl];
        URED_DBG_CHECK((size_t)b * C + c < (size_t)gridDim.y * C);
        s_out[(size_t)b * C + c] = t / (float)N;
    }
}

__global__ __launch_bounds__(VRC_T) void sk_mean_bwd_kernel(const float* __restrict__ y, const float* __restrict__ ds, int N,
                                                            int C, long long total, float* __restrict__ dy) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;
    const long long r = i / C;
    const int c = (int)(i - r * C);
    const long long b = r / N;
    URED_DBG_CHECK((b + 1) * N * C <= total);
    dy[i] = y[i] > 0.f ? ds[b * C + c] / (float)N : 0.f;
}

// out = sum_i a[b][i][c] * max(y_i, 0) (i ascending), then max(., 0) when relu
__global__ __launch_bounds__(VRC_T) void sk_mix_fwd_kernel(Branches Y, const float* __restrict__ a, int m, int N, int C,
                                                           long long total, int relu, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;
    const long long r = i / C;
    const int c = (int)(i - r * C);
    const long long b = r / N;
    float v = 0.f;
    URED_DBG_CHECK((b + 1) * N * C <= total);
    for (int q = 0; q < m; ++q) {
        const float pr = a[(b * m + q) * C + c] * fmaxf(Y.y[q][i], 0.f);
        v = q == 0 ? pr : v + pr;
    }
    out[i] = relu ? fmaxf(v, 0.f) : v;
}

// dy_i = a_i * G where y_i > 0 else 0, G = g where (no relu or out > 0) else 0
__global__ __launch_bounds__(VRC_T) void sk_mix_bwd_y_kernel(const float* __restrict__ g, const float* __restrict__ out,
                                                             Branches Y, const float* __restrict__ a, int m, int N, int C,
                                                             long long total, int relu, BranchesOut D) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;
    const long long r = i / C;
    const int c = (int)(i - r * C);
    const long long b = r / N;
    const float G = (!relu || out[i] > 0.f) ? g[i] : 0.f;
    URED_DBG_CHECK((b + 1) * N * C <= total);
    for (int q = 0; q < m; ++q) D.y[q][i] = Y.y[q][i] > 0.f ? a[(b * m + q) * C + c] * G : 0.f;
}

// da[b][i][c] = sum over n of G[b][n][c] * max(y_i[b][n][c], 0), in the order of sk_mean_fwd_kernel
__global__ __launch_bounds__(VRC_T) void sk_mix_bwd_a_kernel(const float* __restrict__ g, const float* __restrict__ out,
                                                             Branches Y, int m, int N, int C, int relu,
                                                             float* __restrict__ da) {
    __shared__ float part[URED_VRC_MMAX][SK_G][64];
    const int gq = threadIdx.x >> 6, cl = threadIdx.x & 63;
    const int c = blockIdx.x * 64 + cl, b = blockIdx.y;
    float acc[URED_VRC_MMAX];
#pragma unroll
    for (int q = 0; q < URED_VRC_MMAX; ++q) acc[q] = 0.f;
    if (c < C) {
        for (int n = gq; n < N; n += SK_G) {
            const size_t at = ((size_t)b * N + n) * C + c;
            const float G = (!relu || out[at] > 0.f) ? g[at] : 0.f;
#pragma unroll
            for (int q = 0; q < URED_VRC_MMAX; ++q) {
                if (q < m) {
                    const float pr = G * fmaxf(Y.y[q][at], 0.f);
                    acc[q] += pr;
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < URED_VRC_MMAX; ++q) part[q][gq][cl] = acc[q];
    __syncthreads();
    if (gq == 0 && c < C) {
        for (int q = 0; q < m; ++q) {
            float t = part[q][0][cl];
#pragma unroll
            for (int u = 1; u < SK_G; ++u) t += part[q][u][cl];
            URED_DBG_CHECK(((size_t)b * m + q) * C + c < (size_t)gridDim.y * m * C);
            da[((size_t)b * m + q) * C + c] = t;
        }
    }
}

// ---------------- edge-preserved pooling ----------------

__global__ __launch_bounds__(VRC_T) void pool_fwd_kernel(const float* __restrict__ feat, const int* __restrict__ p_idx,
                                                         const int* __restrict__ pn_idx, int N, int S, int pk, int C,
                                                         long long total, float* __restrict__ out,
                                                         unsigned char* __restrict__ slot) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;                           // total = B * S * C
    const long long rs = i / C;                       // b * S + s
    const int c = (int)(i - rs * C);
    const long long b = rs / S;
    const float* F = feat + (size_t)b * N * C;
    const int pc = p_idx[rs];
    URED_DBG_CHECK(pc >= 0 && pc < N && (b + 1) * S * C <= total);
    const float centre = (pc >= 0 && pc < N) ? F[(size_t)pc * C + c] : 0.f;
    float best = 0.f;
    int sl = 0;
    for (int j = 0; j < pk; ++j) {
        const int id = pn_idx[rs * pk + j];
        URED_DBG_CHECK(id >= 0 && id < N);            // the kernel tolerates a bad index (zero row); the encoder never makes one
        const float v = (id >= 0 && id < N) ? F[(size_t)id * C + c] : 0.f;
        if (j == 0 || v > best) {
            best = v;
            sl = j;
        }
    }
    out[(size_t)rs * 2 * C + c] = centre;
    out[(size_t)rs * 2 * C + C + c] = best;
    slot[i] = (unsigned char)sl;
}

// centre entries (ascending s) first, then the neighbour entries in ascending (s, j)
__global__ __launch_bounds__(64) void pool_bwd_kernel(const float* __restrict__ g, const int* __restrict__ p_idx,
                                                      const int* __restrict__ pn_idx, const unsigned char* __restrict__ slot,
                                                      int N, int S, int pk, int C, int tiles_n, float* __restrict__ dfeat) {
    __shared__ float acc[SC_P * SC_C];
    const int ln = threadIdx.x, b = blockIdx.y;
    const int tn = blockIdx.x % tiles_n, tc = blockIdx.x / tiles_n;
    const int j0 = tn * SC_P, c = tc * SC_C + ln;
    const bool cin = c < C;
    const size_t sb = (size_t)b * S;
#pragma unroll
    for (int p = 0; p < SC_P; ++p) acc[p * SC_C + ln] = 0.f;
    scan_add(p_idx + sb, S, j0, ln, acc, [&](int e) -> float { return cin ? g[(sb + e) * 2 * C + c] : 0.f; });
    scan_add(pn_idx + sb * pk, S * pk, j0, ln, acc, [&](int e) -> float {
        if (!cin) return 0.f;
        const int s = e / pk, j = e - s * pk;
        URED_DBG_CHECK(s < S && (int)slot[(sb + s) * C + c] < pk);
        return (int)slot[(sb + s) * C + c] == j ? g[(sb + s) * 2 * C + C + c] : 0.f;
    });
    if (!cin) return;
    for (int p = 0; p < SC_P; ++p) {
        const int m = j0 + p;
        if (m >= N) break;
        URED_DBG_CHECK(((size_t)b * N + m) * C + c < (size_t)gridDim.y * N * C);
        dfeat[((size_t)b * N + m) * C + c] = acc[p * SC_C + ln];
    }
}

// ---------------- three-point unpooling ----------------

// out[r][c] = ((w0 f0 + w1 f1) + w2 f2)[c] for c < D2, skip[r][c - D2] after them
__global__ __launch_bounds__(VRC_T) void unpool_fwd_kernel(const float* __restrict__ feat2, const int* __restrict__ idx,
                                                           const float* __restrict__ w, const float* __restrict__ skip, int N,
                                                           int S, int K, int D2, int D1, long long total,
                                                           float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;                           // total = B * N * (D2 + D1)
    const int Ct = D2 + D1;
    const long long r = i / Ct;
    const int c = (int)(i - r * Ct);
    if (c >= D2) {
        out[i] = skip[r * D1 + (c - D2)];
        return;
    }
    const long long b = r / N;
    float v = 0.f;
    for (int q = 0; q < K; ++q) {
        const int id = idx[r * K + q];
        URED_DBG_CHECK(id >= 0 && id < S);            // tolerated (zero row); three_nn_upsampling never makes one
        const float f = (id >= 0 && id < S) ? feat2[((size_t)b * S + id) * D2 + c] : 0.f;
        const float pr = w[r * K + q] * f;
        v = q == 0 ? pr : v + pr;
    }
    out[i] = v;
}

__global__ __launch_bounds__(64) void unpool_bwd_kernel(const float* __restrict__ g, const int* __restrict__ idx,
                                                        const float* __restrict__ w, int N, int S, int K, int D2, int D1,
                                                        int tiles_s, float* __restrict__ dfeat2) {
    __shared__ float acc[SC_P * SC_C];
    const int ln = threadIdx.x, b = blockIdx.y;
    const int ts = blockIdx.x % tiles_s, tc = blockIdx.x / tiles_s;
    const int j0 = ts * SC_P, c = tc * SC_C + ln;
    const bool cin = c < D2;
    const int Ct = D2 + D1;
    const size_t nb = (size_t)b * N;
#pragma unroll
    for (int p = 0; p < SC_P; ++p) acc[p * SC_C + ln] = 0.f;
    scan_add(idx + nb * K, N * K, j0, ln, acc, [&](int e) -> float {
        if (!cin) return 0.f;
        URED_DBG_CHECK(e / K < N);
        return w[nb * K + e] * g[(nb + e / K) * Ct + c];
    });
    if (!cin) return;
    for (int p = 0; p < SC_P; ++p) {
        const int m = j0 + p;
        if (m >= S) break;
        URED_DBG_CHECK(((size_t)b * S + m) * D2 + c < (size_t)gridDim.y * S * D2);
        dfeat2[((size_t)b * S + m) * D2 + c] = acc[p * SC_C + ln];
    }
}

__global__ __launch_bounds__(VRC_T) void unpool_bwd_skip_kernel(const float* __restrict__ g, int D2, int D1, long long total,
                                                                float* __restrict__ dskip) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;                           // total = B * N * D1
    const long long r = i / D1;
    const int c = (int)(i - r * D1);
    dskip[i] = g[r * (D2 + D1) + D2 + c];
}

// ---------------- EF expansion: edge rows, max over the k slots ----------------

// out[(n k + j)][c] = max((G[(n k + j)][c] + P[n][c]) + P[idx[n][j]][W + c], 0), P [B*N][2 W] = [centre | neighbour];
// without G the first add drops out. An index outside [0, N) reads as a zero neighbour row.
__global__ __launch_bounds__(VRC_T) void ef_edge_fwd_kernel(const float* __restrict__ G, const float* __restrict__ P,
                                                            const int* __restrict__ idx, int N, int k, int W,
                                                            long long total, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;                           // total = B * N * k * W
    const long long e = i / W;                        // (b N + n) k + j
    const int c = (int)(i - e * W);
    const long long rn = e / k;
    const long long b = rn / N;
    const int id = idx[e];
    URED_DBG_CHECK((b + 1) * N * k * W <= total);
    float v = P[rn * 2 * W + c];
    if (G) v = G[i] + v;
    if (id >= 0 && id < N) v += P[(b * N + id) * 2 * W + W + c];
    out[i] = fmaxf(v, 0.f);
}

// With M = g where out > 0 else 0: dG = M (when asked for); dP[n][c] = sum_j M[(n k + j)][c], j ascending.
__global__ __launch_bounds__(VRC_T) void ef_edge_bwd_point_kernel(const float* __restrict__ g, const float* __restrict__ out,
                                                                  int k, int W, long long total, float* __restrict__ dG,
                                                                  float* __restrict__ dP) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;                           // total = B * N * W
    const long long rn = i / W;
    const int c = (int)(i - rn * W);
    float acc = 0.f;
    for (int j = 0; j < k; ++j) {
        const long long at = (rn * k + j) * W + c;
        URED_DBG_CHECK(at < total * k);
        const float m = out[at] > 0.f ? g[at] : 0.f;
        if (dG) dG[at] = m;
        acc += m;
    }
    dP[rn * 2 * W + c] = acc;
}

// dP[m][W + c] = sum over the entries idx[n][j] = m, ascending (n, j), of M[(n k + j)][c]: the ordered scatter
__global__ __launch_bounds__(64) void ef_edge_bwd_scatter_kernel(const float* __restrict__ g, const float* __restrict__ out,
                                                                 const int* __restrict__ idx, int N, int k, int W, int tiles_n,
                                                                 float* __restrict__ dP) {
    __shared__ float acc[SC_P * SC_C];
    const int ln = threadIdx.x, b = blockIdx.y;
    const int tn = blockIdx.x % tiles_n, tc = blockIdx.x / tiles_n;
    const int j0 = tn * SC_P, c = tc * SC_C + ln;
    const bool cin = c < W;
    const size_t eb = (size_t)b * N * k;              // N * k < 2^31 (host check)
#pragma unroll
    for (int p = 0; p < SC_P; ++p) acc[p * SC_C + ln] = 0.f;
    scan_add(idx + eb, N * k, j0, ln, acc, [&](int e) -> float {
        if (!cin) return 0.f;
        const size_t at = (eb + e) * W + c;
        URED_DBG_CHECK(at < (size_t)gridDim.y * N * k * W);
        return out[at] > 0.f ? g[at] : 0.f;
    });
    if (!cin) return;
    for (int p = 0; p < SC_P; ++p) {
        const int m = j0 + p;
        if (m >= N) break;
        const size_t at = ((size_t)b * N + m) * 2 * W + W + c;
        URED_DBG_CHECK(at < (size_t)gridDim.y * N * 2 * W);
        dP[at] = acc[p * SC_C + ln];
    }
}

// H [B*N*k*r][O] read as [n][j][s][c]: out[(n r + s)][c] = max_j H[((n k + j) r + s)][c], the lowest j on a tie
__global__ __launch_bounds__(VRC_T) void ef_max_fwd_kernel(const float* __restrict__ H, int k, int r, int O, long long total,
                                                           float* __restrict__ out, unsigned char* __restrict__ slot) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;                           // total = B * N * r * O
    const long long q = i / O;                        // n r + s
    const int c = (int)(i - q * O);
    const long long n = q / r;
    const int s = (int)(q - n * r);
    float best = 0.f;
    int sl = 0;
    for (int j = 0; j < k; ++j) {
        const long long at = ((n * k + j) * r + s) * O + c;
        URED_DBG_CHECK(at < total * k);
        const float v = H[at];
        if (j == 0 || v > best) {
            best = v;
            sl = j;
        }
    }
    out[i] = best;
    slot[i] = (unsigned char)sl;
}

__global__ __launch_bounds__(VRC_T) void ef_max_bwd_kernel(const float* __restrict__ g, const unsigned char* __restrict__ slot,
                                                           int k, int r, int O, long long total, float* __restrict__ dH) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;                           // total = B * N * k * r * O
    const long long t = i / O;                        // (n k + j) r + s
    const int c = (int)(i - t * O);
    const long long e = t / r;
    const int s = (int)(t - e * r);
    const long long n = e / k;
    const int j = (int)(e - n * k);
    const long long from = (n * r + s) * O + c;
    URED_DBG_CHECK(from * k < total);
    dH[i] = (int)slot[from] == j ? g[from] : 0.f;
}

// ---------------- folding ----------------

// out[(n r + s)][c] = max(U[n][c] + T[s][c], 0)
__global__ __launch_bounds__(VRC_T) void fold_fwd_kernel(const float* __restrict__ U, const float* __restrict__ T, int r, int Co,
                                                         long long total, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;                           // total = B * N * r * Co
    const long long q = i / Co;
    const int c = (int)(i - q * Co);
    const long long n = q / r;
    const int s = (int)(q - n * r);
    out[i] = fmaxf(U[n * Co + c] + T[(long long)s * Co + c], 0.f);
}

// dU[n][c] = sum_s M[(n r + s)][c], s ascending, M = g where out > 0 else 0
__global__ __launch_bounds__(VRC_T) void fold_bwd_u_kernel(const float* __restrict__ g, const float* __restrict__ out, int r,
                                                           int Co, long long total, float* __restrict__ dU) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;                           // total = B * N * Co
    const long long n = i / Co;
    const int c = (int)(i - n * Co);
    float acc = 0.f;
    for (int s = 0; s < r; ++s) {
        const long long at = (n * r + s) * Co + c;
        URED_DBG_CHECK(at < total * r);
        acc += out[at] > 0.f ? g[at] : 0.f;
    }
    dU[i] = acc;
}

// ws[q][s][c] = sum over the points n of chunk q (ascending) of M[(n r + s)][c]; thread = one (s, c)
__global__ __launch_bounds__(VRC_T) void fold_bwd_t_kernel(const float* __restrict__ g, const float* __restrict__ out,
                                                           long long rows, int rc, int chunk, float* __restrict__ ws) {
    const int col = blockIdx.y * VRC_T + threadIdx.x;
    if (col >= rc) return;                            // rc = r * Co
    const long long p0 = (long long)blockIdx.x * chunk;
    const long long p1 = p0 + chunk < rows ? p0 + chunk : rows;
    float acc = 0.f;
    for (long long p = p0; p < p1; ++p) {
        const long long at = p * rc + col;
        acc += out[at] > 0.f ? g[at] : 0.f;
    }
    URED_DBG_CHECK((long long)blockIdx.x * rc + col < (long long)gridDim.x * rc);
    ws[(long long)blockIdx.x * rc + col] = acc;
}

// ---- Model's latent heads (models/vrcnet.py:457-501) ----
// torch's softplus (beta 1, threshold 20) and its derivative z / (z + 1), z = exp(x); 1 above the threshold
__device__ __forceinline__ float softplus20(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float softplus20_grad(float x) {
    if (x > 20.f) return 1.f;
    const float z = expf(x);
    return z / (z + 1.f);
}

// KL(N(mp, sp) || N(mq, sq)) in the form of torch's kl_divergence: r = (sp / sq)^2, t = ((mp - mq) / sq)^2
__device__ __forceinline__ float kl_normal(float mp, float sp, float mq, float sq, float& r, float& t) {
    const float a = sp / sq, d = (mp - mq) / sq;
    r = a * a;
    t = d * d;
    return 0.5f * (((r + t) - 1.f) - logf(r));
}

// thread = one (b, d) of [B][Z]; o rows are [mu (Z) | raw scale (Z)]
__global__ __launch_bounds__(VRC_T) void latent_fwd_kernel(const float* __restrict__ oq, const float* __restrict__ op,
                                                           const float* __restrict__ eq, const float* __restrict__ ep, int Z,
                                                           long long total, float* __restrict__ z, float* __restrict__ kl_rec,
                                                           float* __restrict__ kl_g) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;                           // total = B * Z
    const long long b = i / Z;
    const int d = (int)(i - b * Z);
    const long long at = b * 2 * Z + d;
    URED_DBG_CHECK(at + Z < 2 * total);
    const float mq = oq[at], sq = softplus20(oq[at + Z]);
    z[i] = mq + sq * eq[i];
    if (op) {
        const float mp = op[at], sp = softplus20(op[at + Z]);
        z[total + i] = mp + sp * ep[i];
        float r, t;
        kl_rec[i] = kl_normal(0.f, 1.f, mp, sp, r, t);
        kl_g[i] = kl_normal(mp, sp, mq, sq, r, t);
    }
}

// d kl / d mq = -((mp - mq) / sq) / sq, d kl / d sq = -((r - 1) + t) / sq; kl_g reaches the posterior only, kl_rec the
// prior only; absent cotangents (null) count as zero; every element of d_oq (and d_op) is written
__global__ __launch_bounds__(VRC_T) void latent_bwd_kernel(const float* __restrict__ oq, const float* __restrict__ op,
                                                           const float* __restrict__ eq, const float* __restrict__ ep,
                                                           const float* __restrict__ dz, const float* __restrict__ dkr,
                                                           const float* __restrict__ dkg, int Z, long long total,
                                                           float* __restrict__ d_oq, float* __restrict__ d_op) {
    const long long i = (long long)blockIdx.x * VRC_T + threadIdx.x;
    if (i >= total) return;
    const long long b = i / Z;
    const int d = (int)(i - b * Z);
    const long long at = b * 2 * Z + d;
    URED_DBG_CHECK(at + Z < 2 * total);
    const float mq = oq[at], xq = oq[at + Z], sq = softplus20(xq);
    float dmq = 0.f, dsq = 0.f;
    if (dz) {
        const float g = dz[i];
        dmq = g;
        dsq = g * eq[i];
    }
    if (op) {
        const float mp = op[at], xp = op[at + Z], sp = softplus20(xp);
        float dmp = 0.f, dsp = 0.f;
        if (dz) {
            const float g = dz[total + i];
            dmp = g;
            dsp = g * ep[i];
        }
        if (dkr) {
            float r, t;
            kl_normal(0.f, 1.f, mp, sp, r, t);
            const float g = dkr[i];
            dmp += g * ((mp / sp) / sp);
            dsp += g * (-((r - 1.f) + t) / sp);
        }
        if (dkg) {
            float r, t;
            kl_normal(mp, sp, mq, sq, r, t);
            const float g = dkg[i];
            dmq += g * (-((mp - mq) / sq) / sq);
            dsq += g * (-((r - 1.f) + t) / sq);
        }
        d_op[at] = dmp;
        d_op[at + Z] = dsp * softplus20_grad(xp);
    }
    d_oq[at] = dmq;
    d_oq[at + Z] = dsq * softplus20_grad(xq);
}

// ---- compute_kernel (models/vrcnet.py:430-437) ----
// One wave per pair (i, j): lane l sums (x[i][d] - y[j][d])^2 over d = l, l + 64, .. ascending, the 64 lane
// sums meet in wave_sum's butterfly; K = exp(-(sum / Z) / Z). Equal rows give exp(-0) = 1 exactly.
__global__ __launch_bounds__(VRC_T) void gauss_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, int m,
                                                          int Z, float* __restrict__ K) {
    const long long p = (long long)blockIdx.x * VRC_W + (threadIdx.x >> 6);
    const int ln = threadIdx.x & 63;
    if (p >= (long long)n * m) return;                // whole waves leave; no barrier below
    const int i = (int)(p / m), j = (int)(p - (long long)i * m);
    URED_DBG_CHECK(i < n && j < m);
    const float* xr = x + (size_t)i * Z;
    const float* yr = y + (size_t)j * Z;
    float acc = 0.f;
    for (int d = ln; d < Z; d += 64) {
        const float df = xr[d] - yr[d];
        acc += df * df;
    }
    acc = wave_sum(acc);
    if (ln == 0) K[p] = expf(-(acc / (float)Z) / (float)Z);
}

// thread = one (row, d) of dx [n][Z] then of dy [m][Z]:
//   dx[i][d] = sum_j (dK[i][j] K[i][j] * -coef) * (x[i][d] - y[j][d]), j ascending
//   dy[j][d] = sum_i (dK[i][j] K[i][j] *  coef) * (x[i][d] - y[j][d]), i ascending;  coef = 2 / Z^2
__global__ __launch_bounds__(VRC_T) void gauss_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          const float* __restrict__ K, const float* __restrict__ dK, int n, int m,
                                                          int Z, float coef, float* __restrict__ dx, float* __restrict__ dy) {
    const long long e = (long long)blockIdx.x * VRC_T + threadIdx.x;
    const long long nx = (long long)n * Z, ny = (long long)m * Z;
    if (e >= nx + ny) return;
    float acc = 0.f;
    if (e < nx) {
        const int i = (int)(e / Z), d = (int)(e - (long long)i * Z);
        const float xv = x[e];
        for (int j = 0; j < m; ++j) {
            const size_t at = (size_t)i * m + j;
            acc += ((dK[at] * K[at]) * -coef) * (xv - y[(size_t)j * Z + d]);
        }
        dx[e] = acc;
    } else {
        const long long f = e - nx;
        const int j = (int)(f / Z), d = (int)(f - (long long)j * Z);
        URED_DBG_CHECK(j < m && d < Z);
        const float yv = y[f];
        for (int i = 0; i < n; ++i) {
            const size_t at = (size_t)i * m + j;
            acc += ((dK[at] * K[at]) * coef) * (x[(size_t)i * Z + d] - yv);
        }
        dy[f] = acc;
    }
}

inline unsigned blocks_for(long long n) { return (unsigned)((n + VRC_T - 1) / VRC_T); }
constexpr long long LIM = 1ll << 31;

int latent_check(const char* who, int B, int Z) {
    URED_REQUIRE(Z >= 1 && Z <= URED_VRC_ZMAX, "%s: Z %d outside [1, %d]", who, Z, URED_VRC_ZMAX);
    URED_REQUIRE(B >= 1 && B <= 65535, "%s: B %d outside [1, 65535]", who, B);
    URED_REQUIRE(2ll * B * Z < LIM, "%s: 2 * B * Z = %lld exceeds 2^31 - 1", who, 2ll * B * Z);
    return 0;
}

int gauss_check(const char* who, int n, int m, int Z) {
    URED_REQUIRE(n >= 1 && n <= URED_VRC_GAUSS_MAX && m >= 1 && m <= URED_VRC_GAUSS_MAX, "%s: n %d or m %d outside [1, %d]",
                 who, n, m, URED_VRC_GAUSS_MAX);
    URED_REQUIRE(Z >= 1 && Z <= URED_VRC_ZMAX, "%s: Z %d outside [1, %d]", who, Z, URED_VRC_ZMAX);
    return 0;
}

int ef_edge_check(const char* who, int B, int N, int k, int W) {
    URED_REQUIRE(B >= 0 && N >= 1, "%s: bad sizes B=%d N=%d", who, B, N);
    URED_REQUIRE(k >= 1 && k <= VRC_KMAX, "%s: k %d outside [1, %d]", who, k, VRC_KMAX);
    URED_REQUIRE(k <= N, "%s: k %d exceeds the cloud's %d points", who, k, N);
    URED_REQUIRE(W >= 1 && W <= URED_VRC_OMAX * URED_VRC_RMAX, "%s: width %d outside [1, %d]", who, W,
                 URED_VRC_OMAX * URED_VRC_RMAX);
    URED_REQUIRE(B <= 65535, "%s: B %d exceeds 65535", who, B);
    URED_REQUIRE((long long)B * N * k * W < LIM && (long long)B * N * 2 * W < LIM,
                 "%s: B * N * k * W and 2 * B * N * W must stay below 2^31", who);
    return 0;
}

int ef_max_check(const char* who, int B, int N, int k, int r, int O) {
    URED_REQUIRE(B >= 0 && N >= 1, "%s: bad sizes B=%d N=%d", who, B, N);
    URED_REQUIRE(k >= 1 && k <= VRC_KMAX, "%s: k %d outside [1, %d]", who, k, VRC_KMAX);
    URED_REQUIRE(r >= 1 && r <= URED_VRC_RMAX, "%s: step ratio %d outside [1, %d]", who, r, URED_VRC_RMAX);
    URED_REQUIRE(O >= 1 && O <= URED_VRC_OMAX, "%s: O %d outside [1, %d]", who, O, URED_VRC_OMAX);
    URED_REQUIRE((long long)B * N * k * r * O < LIM, "%s: B * N * k * r * O = %lld exceeds 2^31 - 1", who,
                 (long long)B * N * k * r * O);
    return 0;
}

int fold_check(const char* who, int B, int N, int r, int Co) {
    URED_REQUIRE(B >= 0 && N >= 1 && Co >= 1, "%s: bad sizes B=%d N=%d Co=%d", who, B, N, Co);
    URED_REQUIRE(r >= 1 && r <= URED_VRC_RMAX, "%s: step ratio %d outside [1, %d]", who, r, URED_VRC_RMAX);
    URED_REQUIRE((long long)B * N * r * Co < LIM, "%s: B * N * r * Co = %lld exceeds 2^31 - 1", who, (long long)B * N * r * Co);
    return 0;
}

int sa_check(const char* who, int B, int N, int k, int rel, int mid, int ms) {
    URED_REQUIRE(B >= 0 && N >= 1, "%s: bad sizes B=%d N=%d", who, B, N);
    URED_REQUIRE(k >= 1 && k <= VRC_KMAX, "%s: k %d outside [1, %d]", who, k, VRC_KMAX);
    URED_REQUIRE(k <= N, "%s: k %d exceeds the cloud's %d points", who, k, N);
    URED_REQUIRE(rel >= 1 && rel <= VRC_RELMAX, "%s: rel %d outside [1, %d]", who, rel, VRC_RELMAX);
    URED_REQUIRE(mid >= 1 && mid <= VRC_MIDMAX, "%s: mid %d outside [1, %d]", who, mid, VRC_MIDMAX);
    URED_REQUIRE(ms >= 1 && ms <= VRC_MSMAX && mid % ms == 0, "%s: ms %d must divide mid %d and lie in [1, %d]", who, ms, mid,
                 VRC_MSMAX);
    URED_REQUIRE(B <= 65535, "%s: B %d exceeds 65535", who, B);
    const long long widest = 2ll * rel + mid > (long long)k * ms ? 2ll * rel + mid : (long long)k * ms;
    URED_REQUIRE((long long)B * N * widest < LIM, "%s: B * N * max(2 rel + mid, k ms) = %lld exceeds 2^31 - 1", who,
                 (long long)B * N * widest);
    URED_REQUIRE((long long)N * k < LIM, "%s: N * k exceeds 2^31 - 1", who);
    return 0;
}

int sk_check(const char* who, int m, int B, int N, int C) {
    URED_REQUIRE(m >= 1 && m <= URED_VRC_MMAX, "%s: m %d outside [1, %d]", who, m, URED_VRC_MMAX);
    URED_REQUIRE(B >= 0 && N >= 1 && C >= 1, "%s: bad sizes B=%d N=%d C=%d", who, B, N, C);
    URED_REQUIRE(B <= 65535, "%s: B %d exceeds 65535", who, B);
    URED_REQUIRE((long long)B * N * C < LIM, "%s: B * N * C = %lld exceeds 2^31 - 1", who, (long long)B * N * C);
    return 0;
}

int pool_check(const char* who, int B, int N, int S, int pk, int C) {
    URED_REQUIRE(B >= 0 && N >= 1 && S >= 1 && C >= 1, "%s: bad sizes B=%d N=%d S=%d C=%d", who, B, N, S, C);
    URED_REQUIRE(pk >= 1 && pk <= URED_VRC_PKMAX, "%s: pk %d outside [1, %d]", who, pk, URED_VRC_PKMAX);
    URED_REQUIRE(B <= 65535, "%s: B %d exceeds 65535", who, B);
    URED_REQUIRE((long long)B * N * C < LIM && (long long)B * S * 2 * C < LIM && (long long)B * S * pk < LIM,
                 "%s: B * N * C, 2 * B * S * C and B * S * pk must stay below 2^31", who);
    return 0;
}

int unpool_check(const char* who, int B, int N, int S, int K, int D2, int D1) {
    URED_REQUIRE(B >= 0 && N >= 1 && S >= 1, "%s: bad sizes B=%d N=%d S=%d", who, B, N, S);
    URED_REQUIRE(K >= 1 && K <= 3, "%s: K %d outside [1, 3]", who, K);
    URED_REQUIRE(D2 >= 1 && D1 >= 0, "%s: D2 %d must be at least 1 and D1 %d non-negative", who, D2, D1);
    URED_REQUIRE(B <= 65535, "%s: B %d exceeds 65535", who, B);
    URED_REQUIRE((long long)B * N * ((long long)D2 + D1) < LIM && (long long)B * S * D2 < LIM && (long long)N * K < LIM,
                 "%s: B * N * (D2 + D1), B * S * D2 and N * K must stay below 2^31", who);
    return 0;
}

int fill(Branches& Y, const char* who, int m, const float* y0, const float* y1, const float* y2, const float* y3) {
    const float* all[URED_VRC_MMAX] = {y0, y1, y2, y3};
    for (int q = 0; q < URED_VRC_MMAX; ++q) {
        URED_REQUIRE(q >= m || all[q], "%s: branch %d is null", who, q);
        Y.y[q] = q < m ? all[q] : nullptr;
    }
    return 0;
}

}  // namespace

extern "C" {

int ured_vrc_sa_fwd(const float* P, const int* idx, const float* Wa, const float* Wb, const float* bb, int B, int N, int k,
                    int rel, int mid, int ms, float* o, float* h, float* w, void* stream) {
    ured::clear_error();
    if (const int rc = sa_check("ured_vrc_sa_fwd", B, N, k, rel, mid, ms)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(P && idx && Wa && Wb && bb && o && h && w, "ured_vrc_sa_fwd: null pointer");
    const u32 BN = (u32)B * (u32)N;
    hipLaunchKernelGGL(sa_fwd_kernel, dim3((BN + VRC_W - 1) / VRC_W), dim3(VRC_T), 0, (hipStream_t)stream, P, idx, Wa, Wb, bb,
                       BN, N, k, rel, mid, ms, o, h, w);
    return ured::launch_status("ured_vrc_sa_fwd");
}

int ured_vrc_sa_bwd(const float* go, const float* o, const float* P, const int* idx, const float* Wa, const float* Wb,
                    const float* h, const float* w, int B, int N, int k, int rel, int mid, int ms, int chunk, float* gm,
                    float* dw, float* dh, float* dP, float* wa_ws, void* stream) {
    ured::clear_error();
    if (const int rc = sa_check("ured_vrc_sa_bwd", B, N, k, rel, mid, ms)) return rc;
    URED_REQUIRE(chunk >= 1, "ured_vrc_sa_bwd: chunk %d must be at least 1", chunk);
    if (B == 0) return 0;
    const u32 BN = (u32)B * (u32)N;
    const long long nchunks = ((long long)BN + chunk - 1) / chunk;
    URED_REQUIRE(nchunks * ms * rel * (k + 1) < LIM, "ured_vrc_sa_bwd: the dWa workspace exceeds 2^31 - 1 elements");
    URED_REQUIRE(go && o && P && idx && Wa && Wb && h && w && gm && dw && dh && dP && wa_ws, "ured_vrc_sa_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sa_bwd_point_kernel, dim3((BN + VRC_W - 1) / VRC_W), dim3(VRC_T), 0, st, go, o, P, idx, Wa, Wb, h, BN, N,
                       k, rel, mid, ms, gm, dw, dh, dP);
    const int tiles_n = (N + SC_P - 1) / SC_P, tiles_c = (rel + mid + SC_C - 1) / SC_C;
    hipLaunchKernelGGL(sa_bwd_scatter_kernel, dim3((unsigned)tiles_n * (unsigned)tiles_c, B), dim3(64), 0, st, gm, w, dh, P, idx,
                       Wa, N, k, rel, mid, ms, tiles_n, dP);
    hipLaunchKernelGGL(sa_bwd_wa_kernel, dim3((unsigned)nchunks), dim3(VRC_T), 0, st, dh, P, idx, BN, N, k, rel, mid, ms, chunk,
                       wa_ws);
    return ured::launch_status("ured_vrc_sa_bwd");
}

int ured_vrc_sk_mean_fwd(const float* y0, const float* y1, const float* y2, const float* y3, int m, int B, int N, int C,
                         float* s, void* stream) {
    ured::clear_error();
    if (const int rc = sk_check("ured_vrc_sk_mean_fwd", m, B, N, C)) return rc;
    if (B == 0) return 0;
    Branches Y;
    if (const int rc = fill(Y, "ured_vrc_sk_mean_fwd", m, y0, y1, y2, y3)) return rc;
    URED_REQUIRE(s, "ured_vrc_sk_mean_fwd: null pointer");
    hipLaunchKernelGGL(sk_mean_fwd_kernel, dim3((C + 63) / 64, B), dim3(VRC_T), 0, (hipStream_t)stream, Y, m, N, C, s);
    return ured::launch_status("ured_vrc_sk_mean_fwd");
}

int ured_vrc_sk_mean_bwd(const float* y, const float* ds, int B, int N, int C, float* dy, void* stream) {
    ured::clear_error();
    if (const int rc = sk_check("ured_vrc_sk_mean_bwd", 1, B, N, C)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(y && ds && dy, "ured_vrc_sk_mean_bwd: null pointer");
    const long long total = (long long)B * N * C;
    hipLaunchKernelGGL(sk_mean_bwd_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, (hipStream_t)stream, y, ds, N, C, total, dy);
    return ured::launch_status("ured_vrc_sk_mean_bwd");
}

int ured_vrc_sk_mix_fwd(const float* y0, const float* y1, const float* y2, const float* y3, const float* a, int m, int B, int N,
                        int C, int relu, float* out, void* stream) {
    ured::clear_error();
    if (const int rc = sk_check("ured_vrc_sk_mix_fwd", m, B, N, C)) return rc;
    if (B == 0) return 0;
    Branches Y;
    if (const int rc = fill(Y, "ured_vrc_sk_mix_fwd", m, y0, y1, y2, y3)) return rc;
    URED_REQUIRE(a && out, "ured_vrc_sk_mix_fwd: null pointer");
    const long long total = (long long)B * N * C;
    hipLaunchKernelGGL(sk_mix_fwd_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, (hipStream_t)stream, Y, a, m, N, C, total,
                       relu, out);
    return ured::launch_status("ured_vrc_sk_mix_fwd");
}

int ured_vrc_sk_mix_bwd(const float* g, const float* out, const float* y0, const float* y1, const float* y2, const float* y3,
                        const float* a, int m, int B, int N, int C, int relu, float* dy0, float* dy1, float* dy2, float* dy3,
                        float* da, void* stream) {
    ured::clear_error();
    if (const int rc = sk_check("ured_vrc_sk_mix_bwd", m, B, N, C)) return rc;
    if (B == 0) return 0;
    Branches Y;
    if (const int rc = fill(Y, "ured_vrc_sk_mix_bwd", m, y0, y1, y2, y3)) return rc;
    BranchesOut D;
    float* outs[URED_VRC_MMAX] = {dy0, dy1, dy2, dy3};
    for (int q = 0; q < URED_VRC_MMAX; ++q) {
        URED_REQUIRE(q >= m || outs[q], "ured_vrc_sk_mix_bwd: gradient of branch %d is null", q);
        D.y[q] = q < m ? outs[q] : nullptr;
    }
    URED_REQUIRE(g && a && da && (out || !relu), "ured_vrc_sk_mix_bwd: null pointer");
    const long long total = (long long)B * N * C;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sk_mix_bwd_y_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, st, g, out, Y, a, m, N, C, total, relu, D);
    hipLaunchKernelGGL(sk_mix_bwd_a_kernel, dim3((C + 63) / 64, B), dim3(VRC_T), 0, st, g, out, Y, m, N, C, relu, da);
    return ured::launch_status("ured_vrc_sk_mix_bwd");
}

int ured_vrc_pool_fwd(const float* feat, const int* p_idx, const int* pn_idx, int B, int N, int S, int pk, int C, float* out,
                      unsigned char* slot, void* stream) {
    ured::clear_error();
    if (const int rc = pool_check("ured_vrc_pool_fwd", B, N, S, pk, C)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(feat && p_idx && pn_idx && out && slot, "ured_vrc_pool_fwd: null pointer");
    const long long total = (long long)B * S * C;
    hipLaunchKernelGGL(pool_fwd_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, (hipStream_t)stream, feat, p_idx, pn_idx, N, S,
                       pk, C, total, out, slot);
    return ured::launch_status("ured_vrc_pool_fwd");
}

int ured_vrc_pool_bwd(const float* g, const int* p_idx, const int* pn_idx, const unsigned char* slot, int B, int N, int S,
                      int pk, int C, float* dfeat, void* stream) {
    ured::clear_error();
    if (const int rc = pool_check("ured_vrc_pool_bwd", B, N, S, pk, C)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(g && p_idx && pn_idx && slot && dfeat, "ured_vrc_pool_bwd: null pointer");
    const int tiles_n = (N + SC_P - 1) / SC_P, tiles_c = (C + SC_C - 1) / SC_C;
    hipLaunchKernelGGL(pool_bwd_kernel, dim3((unsigned)tiles_n * (unsigned)tiles_c, B), dim3(64), 0, (hipStream_t)stream, g,
                       p_idx, pn_idx, slot, N, S, pk, C, tiles_n, dfeat);
    return ured::launch_status("ured_vrc_pool_bwd");
}

int ured_vrc_unpool_fwd(const float* feat2, const int* idx, const float* w, const float* skip, int B, int N, int S, int K,
                        int D2, int D1, float* out, void* stream) {
    ured::clear_error();
    if (const int rc = unpool_check("ured_vrc_unpool_fwd", B, N, S, K, D2, D1)) return rc;
    URED_REQUIRE((skip != nullptr) == (D1 > 0), "ured_vrc_unpool_fwd: skip and D1 > 0 go together (D1 %d)", D1);
    if (B == 0) return 0;
    URED_REQUIRE(feat2 && idx && w && out, "ured_vrc_unpool_fwd: null pointer");
    const long long total = (long long)B * N * (D2 + D1);
    hipLaunchKernelGGL(unpool_fwd_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, (hipStream_t)stream, feat2, idx, w, skip, N,
                       S, K, D2, D1, total, out);
    return ured::launch_status("ured_vrc_unpool_fwd");
}

int ured_vrc_unpool_bwd(const float* g, const int* idx, const float* w, int B, int N, int S, int K, int D2, int D1,
                        float* dfeat2, float* dskip, void* stream) {
    ured::clear_error();
    if (const int rc = unpool_check("ured_vrc_unpool_bwd", B, N, S, K, D2, D1)) return rc;
    URED_REQUIRE((dskip != nullptr) == (D1 > 0), "ured_vrc_unpool_bwd: dskip and D1 > 0 go together (D1 %d)", D1);
    if (B == 0) return 0;
    URED_REQUIRE(g && idx && w && dfeat2, "ured_vrc_unpool_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int tiles_s = (S + SC_P - 1) / SC_P, tiles_c = (D2 + SC_C - 1) / SC_C;
    hipLaunchKernelGGL(unpool_bwd_kernel, dim3((unsigned)tiles_s * (unsigned)tiles_c, B), dim3(64), 0, st, g, idx, w, N, S, K, D2,
                       D1, tiles_s, dfeat2);
    if (D1 > 0) {
        const long long total = (long long)B * N * D1;
        hipLaunchKernelGGL(unpool_bwd_skip_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, st, g, D2, D1, total, dskip);
    }
    return ured::launch_status("ured_vrc_unpool_bwd");
}

int ured_vrc_ef_edge_fwd(const float* G, const float* P, const int* idx, int B, int N, int k, int W, float* out, void* stream) {
    ured::clear_error();
    if (const int rc = ef_edge_check("ured_vrc_ef_edge_fwd", B, N, k, W)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(P && idx && out, "ured_vrc_ef_edge_fwd: null pointer");
    const long long total = (long long)B * N * k * W;
    hipLaunchKernelGGL(ef_edge_fwd_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, (hipStream_t)stream, G, P, idx, N, k, W,
                       total, out);
    return ured::launch_status("ured_vrc_ef_edge_fwd");
}

int ured_vrc_ef_edge_bwd(const float* g, const float* out, const int* idx, int B, int N, int k, int W, float* dG, float* dP,
                         void* stream) {
    ured::clear_error();
    if (const int rc = ef_edge_check("ured_vrc_ef_edge_bwd", B, N, k, W)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(g && out && idx && dP, "ured_vrc_ef_edge_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)B * N * W;
    hipLaunchKernelGGL(ef_edge_bwd_point_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, st, g, out, k, W, total, dG, dP);
    const int tiles_n = (N + SC_P - 1) / SC_P, tiles_c = (W + SC_C - 1) / SC_C;
    hipLaunchKernelGGL(ef_edge_bwd_scatter_kernel, dim3((unsigned)tiles_n * (unsigned)tiles_c, B), dim3(64), 0, st, g, out, idx,
                       N, k, W, tiles_n, dP);
    return ured::launch_status("ured_vrc_ef_edge_bwd");
}

int ured_vrc_ef_max_fwd(const float* H, int B, int N, int k, int r, int O, float* out, unsigned char* slot, void* stream) {
    ured::clear_error();
    if (const int rc = ef_max_check("ured_vrc_ef_max_fwd", B, N, k, r, O)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(H && out && slot, "ured_vrc_ef_max_fwd: null pointer");
    const long long total = (long long)B * N * r * O;
    hipLaunchKernelGGL(ef_max_fwd_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, (hipStream_t)stream, H, k, r, O, total, out,
                       slot);
    return ured::launch_status("ured_vrc_ef_max_fwd");
}

int ured_vrc_ef_max_bwd(const float* g, const unsigned char* slot, int B, int N, int k, int r, int O, float* dH, void* stream) {
    ured::clear_error();
    if (const int rc = ef_max_check("ured_vrc_ef_max_bwd", B, N, k, r, O)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(g && slot && dH, "ured_vrc_ef_max_bwd: null pointer");
    const long long total = (long long)B * N * k * r * O;
    hipLaunchKernelGGL(ef_max_bwd_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, (hipStream_t)stream, g, slot, k, r, O, total,
                       dH);
    return ured::launch_status("ured_vrc_ef_max_bwd");
}

int ured_vrc_fold_fwd(const float* U, const float* T, int B, int N, int r, int Co, float* out, void* stream) {
    ured::clear_error();
    if (const int rc = fold_check("ured_vrc_fold_fwd", B, N, r, Co)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(U && T && out, "ured_vrc_fold_fwd: null pointer");
    const long long total = (long long)B * N * r * Co;
    hipLaunchKernelGGL(fold_fwd_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, (hipStream_t)stream, U, T, r, Co, total, out);
    return ured::launch_status("ured_vrc_fold_fwd");
}

int ured_vrc_fold_bwd(const float* g, const float* out, int B, int N, int r, int Co, int chunk, float* dU, float* ws,
                      void* stream) {
    ured::clear_error();
    if (const int rc = fold_check("ured_vrc_fold_bwd", B, N, r, Co)) return rc;
    URED_REQUIRE(chunk >= 1, "ured_vrc_fold_bwd: chunk %d must be at least 1", chunk);
    if (B == 0) return 0;
    const long long rows = (long long)B * N, rc = (long long)r * Co;
    const long long nchunks = (rows + chunk - 1) / chunk;
    URED_REQUIRE(nchunks * rc < LIM, "ured_vrc_fold_bwd: the dT workspace exceeds 2^31 - 1 elements");
    URED_REQUIRE((rc + VRC_T - 1) / VRC_T <= 65535, "ured_vrc_fold_bwd: r * Co = %lld exceeds %d", rc, 65535 * VRC_T);
    URED_REQUIRE(g && out && dU && ws, "ured_vrc_fold_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long total = rows * Co;
    hipLaunchKernelGGL(fold_bwd_u_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, st, g, out, r, Co, total, dU);
    hipLaunchKernelGGL(fold_bwd_t_kernel, dim3((unsigned)nchunks, (unsigned)((rc + VRC_T - 1) / VRC_T)), dim3(VRC_T), 0, st, g,
                       out, rows, (int)rc, chunk, ws);
    return ured::launch_status("ured_vrc_fold_bwd");
}

int ured_vrc_latent_fwd(const float* oq, const float* op, const float* eps_q, const float* eps_p, int B, int Z, float* z,
                        float* kl_rec, float* kl_g, void* stream) {
    ured::clear_error();
    if (const int rc = latent_check("ured_vrc_latent_fwd", B, Z)) return rc;
    URED_REQUIRE(oq && eps_q && z, "ured_vrc_latent_fwd: null pointer");
    URED_REQUIRE(!op || (eps_p && kl_rec && kl_g), "ured_vrc_latent_fwd: the training form needs eps_p, kl_rec and kl_g");
    const long long total = (long long)B * Z;
    hipLaunchKernelGGL(latent_fwd_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, (hipStream_t)stream, oq, op, eps_q, eps_p, Z,
                       total, z, kl_rec, kl_g);
    return ured::launch_status("ured_vrc_latent_fwd");
}

int ured_vrc_latent_bwd(const float* oq, const float* op, const float* eps_q, const float* eps_p, const float* dz,
                        const float* d_kl_rec, const float* d_kl_g, int B, int Z, float* d_oq, float* d_op, void* stream) {
    ured::clear_error();
    if (const int rc = latent_check("ured_vrc_latent_bwd", B, Z)) return rc;
    URED_REQUIRE(oq && eps_q && d_oq, "ured_vrc_latent_bwd: null pointer");
    URED_REQUIRE(!op || (eps_p && d_op), "ured_vrc_latent_bwd: the training form needs eps_p and d_op");
    URED_REQUIRE(op || (!d_kl_rec && !d_kl_g), "ured_vrc_latent_bwd: the evaluation form has no KL cotangents");
    const long long total = (long long)B * Z;
    hipLaunchKernelGGL(latent_bwd_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, (hipStream_t)stream, oq, op, eps_q, eps_p, dz,
                       d_kl_rec, d_kl_g, Z, total, d_oq, d_op);
    return ured::launch_status("ured_vrc_latent_bwd");
}

int ured_vrc_gauss_fwd(const float* x, const float* y, int n, int m, int Z, float* K, void* stream) {
    ured::clear_error();
    if (const int rc = gauss_check("ured_vrc_gauss_fwd", n, m, Z)) return rc;
    URED_REQUIRE(x && y && K, "ured_vrc_gauss_fwd: null pointer");
    const long long pairs = (long long)n * m;
    hipLaunchKernelGGL(gauss_fwd_kernel, dim3((unsigned)((pairs + VRC_W - 1) / VRC_W)), dim3(VRC_T), 0, (hipStream_t)stream, x, y,
                       n, m, Z, K);
    return ured::launch_status("ured_vrc_gauss_fwd");
}

int ured_vrc_gauss_bwd(const float* x, const float* y, const float* K, const float* dK, int n, int m, int Z, float* dx,
                       float* dy, void* stream) {
    ured::clear_error();
    if (const int rc = gauss_check("ured_vrc_gauss_bwd", n, m, Z)) return rc;
    URED_REQUIRE(x && y && K && dK && dx && dy, "ured_vrc_gauss_bwd: null pointer");
    const long long total = ((long long)n + m) * Z;
    const float coef = 2.f / ((float)Z * (float)Z);
    hipLaunchKernelGGL(gauss_bwd_kernel, dim3(blocks_for(total)), dim3(VRC_T), 0, (hipStream_t)stream, x, y, K, dK, n, m, Z, coef,
                       dx, dy);
    return ured::launch_status("ured_vrc_gauss_bwd");
}

}  // extern "C"

URED_DBG_ACCESSOR(ured_dbg_vrc)
