// vn.hip — Vector-Neuron DGCNN layers (the reference's network/VN/vn_layers.py and vn_dgcnn_util.py:
// get_graph_feature + VNLinearLeakyReLU, VNMaxPool, VNStdFeature's frame product, the feature-space
// kNN) without the [B, 2C, 3, N, k] tensors that the torch composition builds and keeps.
// Plain pointers, the caller's stream, no allocation, no host sync, no device state, no float
// atomics; every limit is checked on the host before any device work. A VN feature is point-major
// with the channel innermost, [B, N, 3, C] fp32, so [B*N*3, C] is a GEMM operand; indices are int32
// and local to their cloud. An index outside [0, N) reads as a zero row and takes no gradient.
//
// The linear maps of an edge layer act on [x_j - x_i, x_i], so W . edge = W_a x_j + (W_b - W_a) x_i:
// the caller runs one per-point GEMM uv = x [B*N*3, C] @ [Wf_a; Wd_a; Wf_b - Wf_a; Wd_b - Wd_a]^T and
// the kernels here evaluate everything after it per edge in registers from two gathered rows.
//   edge form  (idx != NULL): uv [B*N*3, 2W], W = Co + Cd, columns [Uf (Co) | Ud (Cd) | Vf (Co) | Vd (Cd)];
//       p = Uf[idx[b,n,j]] + Vf[n], d = Ud[idx[b,n,j]] + Vd[n]
//   point form (idx == NULL, k = 1): uv [B*N*3, W], columns [P (Co) | D (Cd)]; p = P[n], d = D[n]
//   Cd = Co (a direction per channel) or 1 (shared).
//
// Arithmetic contract (the file is built with -ffp-contract=off and spells the order out), per
// (b, n, j, c) with p, d in R^3:
//   nrm = sqrt(((px*px) + (py*py)) + (pz*pz)) + 1e-6
//   nb  = nrm * scale[c] + shift[c]       scale = gamma * invstd, shift = beta - mean * scale; training:
//         mean / biased variance of nrm over all B*N*k edges, accumulated in float64 in a fixed order;
//         eval: the running statistics
//   ph  = (p / nrm) * nb
//   t   = ((ph.x*d.x) + (ph.y*d.y)) + (ph.z*d.z),  q = (((d.x*d.x) + (d.y*d.y)) + (d.z*d.z)) + 1e-6
//   mask = t >= 0;  out = mask ? ph : 0.2 * ph + 0.8 * (ph - (t / q) * d)
//   pool mean: out[b,n,:,c] = (sum over ascending j) / k;  pool none: the per-edge tensor [B,N,k,3,Co]
//
// ured_vn_act_fwd.  Training: a statistics pass (lanes across 64 channels, workgroup (x, y) walks a
// contiguous range of points for channel chunk y, the four waves combine through LDS in wave order,
// a finalize kernel adds the partial rows in ascending order, writes mean / invstd / scale / shift
// and updates the running statistics as nn.BatchNorm does). Then one wave per point: neighbours in
// ascending j, channel chunks of 64 inside.
//
// ured_vn_act_bwd.  The branch comes from the saved mask. A statistics pass of the same shape gives
// sum(g_nb) and sum(g_nb * nhat) per channel (grad_beta, grad_gamma, and the two means of the
// BatchNorm backward). The main pass, one wave per point, writes the gradient of (p, d) per edge
// into the caller's edge workspace [B*N*k, 3, W] and their sum over j into the V columns of grad_uv;
// a shared direction's gradient is summed over channels per lane in chunk order and then across the
// wave by a fixed butterfly. The scatter to rows idx[b,n,j] is the scan of group.hip's
// group_bwd_kernel: one wave per (32 target rows, 64 of the 3*W columns) of a cloud walks the cloud's
// N*k indices in ascending order and adds the entries that land in its rows, in that order. Every
// element of grad_uv is written once; a second run is bitwise equal.
//
// ured_vn_knn.  The cloud's [N, N] matrix of squared distances (each summed over ascending d from 0) in
// the caller's workspace, tiled 64 x 64 through LDS, then one wave per row selects the K smallest
// (distance, index) pairs in K rounds of a lexicographic minimum.
//
// ured_vn_maxpool_fwd / _bwd, ured_vn_frame_fwd / _bwd: one thread per (point, channel) and one wave
// per point.
#include <hip/hip_runtime.h>
#define URED_DBG_FILE 15
#include "ured_common.h"
#include "../../include/ured_hip.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned char u8;

constexpr int VN_T = 256;                   // 4 waves: 4 points per workgroup
constexpr int VN_W = VN_T / 64;
constexpr int VN_CH = URED_VN_COMAX / 64;   // channel chunks of a wave
constexpr int VN_P = 32, VN_C = 64;         // target rows x columns of one scatter wave
constexpr float VN_EPS = 1e-6f;

struct VnShape {
    int BN, N, k, Co, Cd, W, LD, edge;
};

// p and d of edge (row, id) for feature column cf and direction column cd
__device__ __forceinline__ void vn_load(const float* __restrict__ uv, const VnShape& s, size_t rowV, size_t rowU, bool ok,
                                        int cf, int cd, float p[3], float d[3]) {
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) {
        const float* V = uv + (rowV * 3 + kk) * (size_t)s.LD;
        if (s.edge) {
            const float* U = uv + (rowU * 3 + kk) * (size_t)s.LD;
            p[kk] = (ok ? U[cf] : 0.f) + V[s.W + cf];
            d[kk] = (ok ? U[s.Co + cd] : 0.f) + V[s.W + s.Co + cd];
        } else {
            p[kk] = V[cf];
            d[kk] = V[s.Co + cd];
        }
    }
}

__device__ __forceinline__ float vn_pnorm(const float p[3]) { return __fsqrt_rn(((p[0] * p[0]) + (p[1] * p[1])) + (p[2] * p[2])); }
__device__ __forceinline__ float vn_dot(const float a[3], const float b[3]) { return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2]); }

__device__ __forceinline__ float vn_wave_sum(float v) {      // a fixed butterfly: the same order every run
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Partial sums of nrm and nrm^2: ws[x][0 | 1][c] (float64), workgroup x covers rows_per_block points.
__global__ __launch_bounds__(VN_T) void vn_stat_fwd_kernel(const float* __restrict__ uv, const int* __restrict__ idx, VnShape s,
                                                           int rows_per_block, double* __restrict__ ws) {
    __shared__ double part[VN_W][2][64];
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + ln;
    const bool cin = c < s.Co;
    const int cc = cin ? c : 0, cd = s.Cd == 1 ? 0 : cc;
    double s1 = 0.0, s2 = 0.0;
    const int r0 = blockIdx.x * rows_per_block;
    for (int t = wv; t < rows_per_block; t += VN_W) {
        const int row = __builtin_amdgcn_readfirstlane(r0 + t);
        if (row >= s.BN) break;                              // wave-uniform
        const size_t base = (size_t)(row / s.N) * s.N;
        for (int j = 0; j < s.k; ++j) {
            const int id = s.edge ? __builtin_amdgcn_readfirstlane(idx[(size_t)row * s.k + j]) : 0;
            const bool ok = (u32)id < (u32)s.N;
            float p[3], d[3];
            vn_load(uv, s, row, base + (ok ? id : 0), ok, cc, cd, p, d);
            const float nrm = vn_pnorm(p) + VN_EPS;
            s1 += (double)nrm;
            s2 += (double)nrm * (double)nrm;
        }
    }
    part[wv][0][ln] = s1; part[wv][1][ln] = s2;
    __syncthreads();
    if (wv != 0 || !cin) return;
    double a = part[0][0][ln], b = part[0][1][ln];
#pragma unroll
    for (int w = 1; w < VN_W; ++w) { a += part[w][0][ln]; b += part[w][1][ln]; }
    ws[((size_t)blockIdx.x * 2) * s.Co + c] = a;
    ws[((size_t)blockIdx.x * 2 + 1) * s.Co + c] = b;
}

// stat [4][Co] = mean, invstd, scale, shift. Training (ws != NULL): from the partial rows, and the
// running statistics move; eval: from the running statistics.
__global__ __launch_bounds__(VN_T) void vn_stat_finalize_kernel(const double* __restrict__ ws, int parts, int Co, double M,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                float* __restrict__ rmean, float* __restrict__ rvar,
                                                                long long* __restrict__ nbt, float momentum, float eps,
                                                                float* __restrict__ stat) {
    const int c = blockIdx.x * VN_T + threadIdx.x;
    if (c == 0 && ws && nbt) *nbt += 1;
    if (c >= Co) return;
    double mean, var;
    if (ws) {
        double a = 0.0, b = 0.0;
        for (int p = 0; p < parts; ++p) { a += ws[((size_t)p * 2) * Co + c]; b += ws[((size_t)p * 2 + 1) * Co + c]; }
        mean = a / M;
        var = b / M - mean * mean;
        var = var > 0.0 ? var : 0.0;
        if (rmean) rmean[c] = (float)((1.0 - (double)momentum) * (double)rmean[c] + (double)momentum * mean);
        if (rvar) rvar[c] = (float)((1.0 - (double)momentum) * (double)rvar[c] + (double)momentum * (var * (M / (M - 1.0))));
    } else {
        mean = (double)rmean[c];
        var = (double)rvar[c];
    }
    const double invstd = 1.0 / sqrt(var + (double)eps);
    const double scale = (double)gamma[c] * invstd;
    stat[c] = (float)mean;
    stat[Co + c] = (float)invstd;
    stat[2 * Co + c] = (float)scale;
    stat[3 * Co + c] = (float)((double)beta[c] - mean * scale);
}

// ph, t, q of one (edge, channel); returns the branch.
__device__ __forceinline__ bool vn_act(const float p[3], const float d[3], float nrm, float nb, float ph[3], float& t, float& q) {
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) ph[kk] = __fdiv_rn(p[kk], nrm) * nb;
    t = vn_dot(ph, d);
    q = vn_dot(d, d) + VN_EPS;
    return t >= 0.f;
}

// NCH = ceil(Co / 64) channel chunks per lane: the accumulators are sized for the layer, not for COMAX.
template <int NCH>
__global__ __launch_bounds__(VN_T) void vn_act_fwd_kernel(const float* __restrict__ uv, const int* __restrict__ idx, VnShape s,
                                                          const float* __restrict__ stat, int pool_mean,
                                                          float* __restrict__ out, u8* __restrict__ mask) {
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * VN_W + wv);
    if (row >= s.BN) return;
    const size_t base = (size_t)(row / s.N) * s.N;
    float acc[NCH][3];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) acc[ch][0] = acc[ch][1] = acc[ch][2] = 0.f;
    for (int j = 0; j < s.k; ++j) {
        const int id = s.edge ? __builtin_amdgcn_readfirstlane(idx[(size_t)row * s.k + j]) : 0;
        const bool ok = (u32)id < (u32)s.N;
        const size_t e = (size_t)row * s.k + j;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            if (ch * 64 < s.Co) {
                const int c = ch * 64 + ln;
                const bool cin = c < s.Co;
                const int cc = cin ? c : 0, cd = s.Cd == 1 ? 0 : cc;
                float p[3], d[3], ph[3], t, q;
                vn_load(uv, s, row, base + (ok ? id : 0), ok, cc, cd, p, d);
                const float nrm = vn_pnorm(p) + VN_EPS;
                const float nb = nrm * stat[2 * s.Co + cc] + stat[3 * s.Co + cc];
                const bool m = vn_act(p, d, nrm, nb, ph, t, q);
                const float sq = __fdiv_rn(t, q);
                if (cin) {
                    URED_DBG_CHECK(e < (size_t)s.BN * s.k);
                    mask[e * s.Co + c] = m ? 1 : 0;
#pragma unroll
                    for (int kk = 0; kk < 3; ++kk) {
                        const float o = m ? ph[kk] : 0.2f * ph[kk] + 0.8f * (ph[kk] - sq * d[kk]);
                        if (pool_mean) acc[ch][kk] += o;
                        else out[(e * 3 + kk) * s.Co + c] = o;
                    }
                }
            }
        }
    }
    if (!pool_mean) return;
    const float kf = (float)s.k;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int c = ch * 64 + ln;
        if (c < s.Co) {
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) out[((size_t)row * 3 + kk) * s.Co + c] = __fdiv_rn(acc[ch][kk], kf);
        }
    }
}

// Everything the backward needs of one (edge, channel): the gradient of ph and d from the upstream
// gradient go of out, and g_nb = (g_ph . p) / nrm with nhat = (nrm - mean) * invstd.
struct VnBwd {
    float p[3], d[3], ph[3], gph[3], gd[3];
    float pn, nrm, nb, gr, gnb, nhat;
};

__device__ __forceinline__ void vn_bwd_eval(VnBwd& v, const float go[3], bool m, const float* __restrict__ stat, int Co, int cc) {
    v.pn = vn_pnorm(v.p);
    v.nrm = v.pn + VN_EPS;
    v.nb = v.nrm * stat[2 * Co + cc] + stat[3 * Co + cc];
    float t, q;
    vn_act(v.p, v.d, v.nrm, v.nb, v.ph, t, q);
    if (m) {
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) { v.gph[kk] = go[kk]; v.gd[kk] = 0.f; }
    } else {
        // out = ph - 0.8 * s * d, s = t / q
        const float sq = __fdiv_rn(t, q);
        const float gs = -0.8f * vn_dot(go, v.d);
        const float gt = __fdiv_rn(gs, q);                    // d s / d t = 1 / q
        const float gq = -(gt * sq);                          // d s / d q = -s / q
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) {
            v.gph[kk] = go[kk] + gt * v.d[kk];
            v.gd[kk] = ((-0.8f * sq) * go[kk] + gt * v.ph[kk]) + (2.f * gq) * v.d[kk];
        }
    }
    v.gr = vn_dot(v.gph, v.p);                                // ph = p * r, r = nb / nrm
    v.gnb = __fdiv_rn(v.gr, v.nrm);
    v.nhat = (v.nrm - stat[cc]) * stat[Co + cc];
}

__device__ __forceinline__ void vn_load_go(const float* __restrict__ g, const VnShape& s, size_t row, size_t e, int c,
                                           int pool_mean, float go[3]) {
#pragma unroll
    for (int kk = 0; kk < 3; ++kk)
        go[kk] = pool_mean ? __fdiv_rn(g[(row * 3 + kk) * s.Co + c], (float)s.k) : g[(e * 3 + kk) * s.Co + c];
}

// Partial sums of g_nb and g_nb * nhat: ws[x][0 | 1][c] (float64).
__global__ __launch_bounds__(VN_T) void vn_stat_bwd_kernel(const float* __restrict__ g, const float* __restrict__ uv,
                                                           const int* __restrict__ idx, const u8* __restrict__ mask, VnShape s,
                                                           const float* __restrict__ stat, int pool_mean, int rows_per_block,
                                                           double* __restrict__ ws) {
    __shared__ double part[VN_W][2][64];
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + ln;
    const bool cin = c < s.Co;
    const int cc = cin ? c : 0, cd = s.Cd == 1 ? 0 : cc;
    double s1 = 0.0, s2 = 0.0;
    const int r0 = blockIdx.x * rows_per_block;
    for (int t = wv; t < rows_per_block; t += VN_W) {
        const int row = __builtin_amdgcn_readfirstlane(r0 + t);
        if (row >= s.BN) break;                              // wave-uniform
        const size_t base = (size_t)(row / s.N) * s.N;
        for (int j = 0; j < s.k; ++j) {
            const int id = s.edge ? __builtin_amdgcn_readfirstlane(idx[(size_t)row * s.k + j]) : 0;
            const bool ok = (u32)id < (u32)s.N;
            const size_t e = (size_t)row * s.k + j;
            VnBwd v;
            float go[3];
            vn_load(uv, s, row, base + (ok ? id : 0), ok, cc, cd, v.p, v.d);
            vn_load_go(g, s, row, e, cc, pool_mean, go);
            vn_bwd_eval(v, go, mask[e * s.Co + cc] != 0, stat, s.Co, cc);
            s1 += (double)v.gnb;
            s2 += (double)v.gnb * (double)v.nhat;
        }
    }
    part[wv][0][ln] = s1; part[wv][1][ln] = s2;
    __syncthreads();
    if (wv != 0 || !cin) return;
    double a = part[0][0][ln], b = part[0][1][ln];
#pragma unroll
    for (int w = 1; w < VN_W; ++w) { a += part[w][0][ln]; b += part[w][1][ln]; }
    ws[((size_t)blockIdx.x * 2) * s.Co + c] = a;
    ws[((size_t)blockIdx.x * 2 + 1) * s.Co + c] = b;
}

// grad_beta = sum g_nb, grad_gamma = sum g_nb * nhat; coef [2][Co] = their means in training, 0 in eval.
__global__ __launch_bounds__(VN_T) void vn_stat_bwd_finalize_kernel(const double* __restrict__ ws, int parts, int Co, double M,
                                                                    int training, float* __restrict__ grad_gamma,
                                                                    float* __restrict__ grad_beta, float* __restrict__ coef) {
    const int c = blockIdx.x * VN_T + threadIdx.x;
    if (c >= Co) return;
    double a = 0.0, b = 0.0;
    for (int p = 0; p < parts; ++p) { a += ws[((size_t)p * 2) * Co + c]; b += ws[((size_t)p * 2 + 1) * Co + c]; }
    grad_beta[c] = (float)a;
    grad_gamma[c] = (float)b;
    coef[c] = training ? (float)(a / M) : 0.f;
    coef[Co + c] = training ? (float)(b / M) : 0.f;
}

template <int NCH>
__global__ __launch_bounds__(VN_T) void vn_act_bwd_kernel(const float* __restrict__ g, const float* __restrict__ uv,
                                                          const int* __restrict__ idx, const u8* __restrict__ mask, VnShape s,
                                                          const float* __restrict__ stat, const float* __restrict__ coef,
                                                          int pool_mean, float* __restrict__ edge_ws, float* __restrict__ grad_uv) {
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * VN_W + wv);
    if (row >= s.BN) return;
    const size_t base = (size_t)(row / s.N) * s.N;
    const bool shared = s.Cd == 1;
    const int voff = s.edge ? s.W : 0;                       // the V (or point) columns of grad_uv
    float ap[NCH][3], ad[NCH][3], as[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) { ap[ch][0] = ap[ch][1] = ap[ch][2] = 0.f; ad[ch][0] = ad[ch][1] = ad[ch][2] = 0.f; }
    for (int j = 0; j < s.k; ++j) {
        const int id = s.edge ? __builtin_amdgcn_readfirstlane(idx[(size_t)row * s.k + j]) : 0;
        const bool ok = (u32)id < (u32)s.N;
        const size_t e = (size_t)row * s.k + j;
        float sd[3] = {0.f, 0.f, 0.f};                       // the lane's share of a shared direction's gradient
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            if (ch * 64 < s.Co) {
                const int c = ch * 64 + ln;
                const bool cin = c < s.Co;
                const int cc = cin ? c : 0, cd = shared ? 0 : cc;
                VnBwd v;
                float go[3];
                vn_load(uv, s, row, base + (ok ? id : 0), ok, cc, cd, v.p, v.d);
                vn_load_go(g, s, row, e, cc, pool_mean, go);
                vn_bwd_eval(v, go, mask[e * s.Co + cc] != 0, stat, s.Co, cc);
                // nrm = |p| + eps reaches p through r = nb / nrm and through the BatchNorm
                const float gn = -__fdiv_rn(v.gr * v.nb, v.nrm * v.nrm);
                const float gbn = stat[2 * s.Co + cc] * ((v.gnb - coef[cc]) - v.nhat * coef[s.Co + cc]);
                const float gnt = gn + gbn;
                const float r = __fdiv_rn(v.nb, v.nrm);
                if (cin) {
#pragma unroll
                    for (int kk = 0; kk < 3; ++kk) {
                        const float dir = v.pn > 0.f ? __fdiv_rn(v.p[kk], v.pn) : 0.f;   // |p| has gradient 0 at p = 0
                        const float gp = v.gph[kk] * r + gnt * dir;
                        ap[ch][kk] += gp;
                        if (s.edge) edge_ws[(e * 3 + kk) * s.W + c] = gp;
                        if (shared) sd[kk] += v.gd[kk];
                        else {
                            ad[ch][kk] += v.gd[kk];
                            if (s.edge) edge_ws[(e * 3 + kk) * s.W + s.Co + c] = v.gd[kk];
                        }
                    }
                }
            }
        }
        if (shared) {
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
                const float tot = vn_wave_sum(sd[kk]);
                as[kk] += tot;
                if (s.edge && ln == 0) edge_ws[(e * 3 + kk) * s.W + s.Co] = tot;
            }
        }
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int c = ch * 64 + ln;
        if (c < s.Co) {
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
                float* G = grad_uv + ((size_t)row * 3 + kk) * s.LD + voff;
                G[c] = ap[ch][kk];
                if (!shared) G[s.Co + c] = ad[ch][kk];
            }
        }
    }
    if (shared && ln == 0) {
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) grad_uv[((size_t)row * 3 + kk) * s.LD + voff + s.Co] = as[kk];
    }
}

// The U columns of grad_uv: entries e = 0..N*k-1 of cloud b in ascending order, each added to row
// idx[e] of the lane's column (kk, w) of the 3*W.
__global__ __launch_bounds__(64) void vn_scatter_kernel(const float* __restrict__ edge_ws, const int* __restrict__ idx, int N,
                                                        int k, int W, int LD, float* __restrict__ grad_uv) {
    __shared__ float acc[VN_P * VN_C];                       // column ln belongs to lane ln alone: no barrier anywhere
    const int ln = threadIdx.x, b = blockIdx.z, j0 = blockIdx.x * VN_P, col = blockIdx.y * VN_C + ln;
    const bool cin = col < 3 * W;
    const int kk = cin ? col / W : 0, w = cin ? col - kk * W : 0;
    const size_t base = (size_t)b * N;
    const int* I = idx + base * k;
    const int E = N * k;
#pragma unroll
    for (int p = 0; p < VN_P; ++p) acc[p * VN_C + ln] = 0.f;
    for (int e0 = 0; e0 < E; e0 += 64) {
        const int e = e0 + ln;
        const int id = e < E ? I[e] : -1;
        const int pl = (u32)id < (u32)N ? id - j0 : -1;
        u64 hit = __ballot((u32)pl < (u32)VN_P);
        while (hit) {                                        // the wave's entries of this batch, ascending
            const int l = (int)__builtin_ctzll(hit);
            hit &= hit - 1;
            const int p = __builtin_amdgcn_readlane(pl, l);
            URED_DBG_CHECK(p >= 0 && p < VN_P && e0 + l < E);
            if (cin) acc[p * VN_C + ln] += edge_ws[((base * k + (size_t)(e0 + l)) * 3 + kk) * W + w];
        }
    }
    if (!cin) return;
    for (int p = 0; p < VN_P; ++p) {
        const int r = j0 + p;
        if (r >= N) break;
        grad_uv[((base + r) * 3 + kk) * LD + w] = acc[p * VN_C + ln];
    }
}

// ---------------- kNN in D dimensions ----------------

// Two launches. vn_knn_dist_kernel: a 256-thread workgroup computes a 64 x 64 tile of the cloud's
// [N, N] distance matrix, 4 x 4 entries per thread, from query and candidate rows staged transposed in
// LDS 32 dimensions at a time; every entry is its own sum over ascending d from 0, so the tiling does
// not touch the contract's order. vn_knn_select_kernel: one wave per query row picks the K smallest
// (distance, index) pairs in K rounds; a round takes the lexicographic minimum of the pairs that follow
// the previous round's pick (per lane over i = lane, lane + 64, ..., then a butterfly), so no list is
// kept and any N works. A row without K comparable distances (NaN) ends in -1 entries.
constexpr int KN_T = 64, KN_D = 32, KN_S = KN_T + 1;         // tile edge, dimensions per stage, LDS row stride

__global__ __launch_bounds__(256) void vn_knn_dist_kernel(const float* __restrict__ x, int N, int D, float* __restrict__ dist) {
    __shared__ float qs[KN_D * KN_S], cs[KN_D * KN_S];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int b = blockIdx.z, q0 = blockIdx.y * KN_T, c0 = blockIdx.x * KN_T;
    const float* X = x + (size_t)b * N * D;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[a][e] = 0.f;
    for (int d0 = 0; d0 < D; d0 += KN_D) {
        const int nd = D - d0 < KN_D ? D - d0 : KN_D;
        for (int t = tid; t < KN_T * KN_D; t += 256) {       // 32 consecutive floats of a row per half-wave
            const int r = t / KN_D, dd = t - r * KN_D;
            const bool din = d0 + dd < D;
            qs[dd * KN_S + r] = din && q0 + r < N ? X[(size_t)(q0 + r) * D + d0 + dd] : 0.f;
            cs[dd * KN_S + r] = din && c0 + r < N ? X[(size_t)(c0 + r) * D + d0 + dd] : 0.f;
        }
        __syncthreads();
        for (int dd = 0; dd < nd; ++dd) {
            float q[4], c[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { q[a] = qs[dd * KN_S + ty * 4 + a]; c[a] = cs[dd * KN_S + tx + 16 * a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float df = c[e] - q[a];
                    acc[a][e] = acc[a][e] + df * df;
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int qi = q0 + ty * 4 + a;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ci = c0 + tx + 16 * e;
            if (qi < N && ci < N) dist[((size_t)b * N + qi) * N + ci] = acc[a][e];
        }
    }
}

__global__ __launch_bounds__(VN_T) void vn_knn_select_kernel(const float* __restrict__ dist, int BN, int N, int K,
                                                             int* __restrict__ idx) {
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int row = __builtin_amdgcn_readfirstlane(blockIdx.x * VN_W + wv);
    if (row >= BN) return;
    const float* R = dist + (size_t)row * N;
    constexpr int NONE = 0x7fffffff;
    float pd = -1.f;                                         // distances are >= 0: every pair follows (-1, -1)
    int pi = -1;
    for (int t = 0; t < K; ++t) {
        float bd = __builtin_inff();
        int bi = NONE;
        for (int i = ln; i < N; i += 64) {
            const float d = R[i];
            const bool after = d > pd || (d == pd && i > pi);
            const bool less = d < bd || (d == bd && i < bi);
            if (after && less) { bd = d; bi = i; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float od = __shfl_xor(bd, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
        }
        URED_DBG_CHECK(bi == NONE || (bi >= 0 && bi < N));
        if (ln == 0) idx[(size_t)row * K + t] = bi == NONE ? -1 : bi;
        pd = bd; pi = bi;
    }
}

// ---------------- VNMaxPool ----------------

__global__ __launch_bounds__(VN_T) void vn_maxpool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ d, int k,
                                                              int C, u32 total, float* __restrict__ out, u8* __restrict__ slot) {
    const u32 e = blockIdx.x * (u32)VN_T + threadIdx.x;      // B * N * C < 2^31 (host check)
    if (e >= total) return;
    const size_t r = e / (u32)C;                             // b * N + n
    const int c = (int)(e - (u32)r * (u32)C);
    float best = 0.f;
    int bj = 0;
    for (int j = 0; j < k; ++j) {
        const size_t o = ((r * k + j) * 3) * C + c;
        const float t = ((x[o] * d[o]) + (x[o + C] * d[o + C])) + (x[o + 2 * (size_t)C] * d[o + 2 * (size_t)C]);
        const bool up = j == 0 || t > best;                  // strict: the lowest j wins a tie
        best = up ? t : best;
        bj = up ? j : bj;
    }
    const size_t o = ((r * k + bj) * 3) * C + c;
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) out[(r * 3 + kk) * C + c] = x[o + (size_t)kk * C];
    slot[e] = (u8)bj;
}

__global__ __launch_bounds__(VN_T) void vn_maxpool_bwd_kernel(const float* __restrict__ g, const u8* __restrict__ slot, int k,
                                                              int C, u32 total, float* __restrict__ gx) {
    const u32 e = blockIdx.x * (u32)VN_T + threadIdx.x;
    if (e >= total) return;
    const size_t r = e / (u32)C;
    const int c = (int)(e - (u32)r * (u32)C);
    const int bj = slot[e];
    URED_DBG_CHECK(bj < k);
    for (int j = 0; j < k; ++j) {
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) gx[((r * k + j) * 3 + kk) * C + c] = j == bj ? g[(r * 3 + kk) * C + c] : 0.f;
    }
}

// ---------------- VNStdFeature's frame product ----------------

// out[r, kk, c] = sum_j x[r, j, c] * z[r, j, kk]
__global__ __launch_bounds__(VN_T) void vn_frame_fwd_kernel(const float* __restrict__ x, const float* __restrict__ z, int C,
                                                            u32 total, float* __restrict__ out) {
    const u32 e = blockIdx.x * (u32)VN_T + threadIdx.x;      // rows * C < 2^31 (host check)
    if (e >= total) return;
    const size_t r = e / (u32)C;
    const int c = (int)(e - (u32)r * (u32)C);
    const float* Z = z + r * 9;
    const float x0 = x[(r * 3) * C + c], x1 = x[(r * 3 + 1) * C + c], x2 = x[(r * 3 + 2) * C + c];
#pragma unroll
    for (int kk = 0; kk < 3; ++kk) out[(r * 3 + kk) * C + c] = ((x0 * Z[kk]) + (x1 * Z[3 + kk])) + (x2 * Z[6 + kk]);
}

// gx[r, j, c] = sum_kk g[r, kk, c] * z[r, j, kk];  gz[r, j, kk] = sum_c x[r, j, c] * g[r, kk, c]: one
// wave per row, the lane's channels in ascending order, then the butterfly.
__global__ __launch_bounds__(VN_T) void vn_frame_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                            const float* __restrict__ z, int rows, int C, float* __restrict__ gx,
                                                            float* __restrict__ gz) {
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = __builtin_amdgcn_readfirstlane(blockIdx.x * VN_W + wv);
    if (r >= rows) return;
    const float* Z = z + (size_t)r * 9;
    float a[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) a[i] = 0.f;
    for (int c = ln; c < C; c += 64) {
        float gv[3], xv[3];
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) {
            gv[kk] = g[((size_t)r * 3 + kk) * C + c];
            xv[kk] = x[((size_t)r * 3 + kk) * C + c];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            gx[((size_t)r * 3 + j) * C + c] = ((gv[0] * Z[3 * j]) + (gv[1] * Z[3 * j + 1])) + (gv[2] * Z[3 * j + 2]);
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) a[3 * j + kk] += xv[j] * gv[kk];
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const float tot = vn_wave_sum(a[i]);
        if (ln == 0) gz[(size_t)r * 9 + i] = tot;
    }
}

int vn_check(const char* who, int B, int N, int k, int Co, int Cd, bool edge) {
    URED_REQUIRE(B >= 0, "%s: negative size (B %d)", who, B);
    URED_REQUIRE(N >= 1, "%s: N %d must be at least 1", who, N);
    URED_REQUIRE(k >= 1 && k <= URED_VN_KMAX, "%s: k %d outside [1, %d]", who, k, URED_VN_KMAX);
    URED_REQUIRE(edge || k == 1, "%s: the point form (idx == NULL) has k = 1, got %d", who, k);
    URED_REQUIRE(Co >= 1 && Co <= URED_VN_COMAX, "%s: Co %d outside [1, %d]", who, Co, URED_VN_COMAX);
    URED_REQUIRE(Cd == Co || Cd == 1, "%s: Cd %d must be Co %d (per channel) or 1 (shared)", who, Cd, Co);
    URED_REQUIRE(B <= 65535, "%s: B %d exceeds 65535", who, B);
    URED_REQUIRE((long long)B * N * k * 3 * 2 * (Co + Cd) < (1ll << 31), "%s: B * N * k * 6 * (Co + Cd) = %lld exceeds 2^31 - 1",
                 who, (long long)B * N * k * 3 * 2 * (Co + Cd));
    return 0;
}

VnShape vn_shape(int B, int N, int k, int Co, int Cd, bool edge) {
    VnShape s;
    s.BN = B * N; s.N = N; s.k = k; s.Co = Co; s.Cd = Cd; s.W = Co + Cd; s.LD = edge ? 2 * s.W : s.W; s.edge = edge ? 1 : 0;
    return s;
}

int rows_check(const char* who, long long rows, int C) {
    URED_REQUIRE(rows >= 0 && C >= 1, "%s: negative size (rows %lld) or C %d below 1", who, rows, C);
    URED_REQUIRE(rows * 3 * C < (1ll << 31), "%s: rows * 3 * C = %lld exceeds 2^31 - 1", who, rows * 3 * C);
    return 0;
}

}  // namespace

extern "C" {

// 1, 2 or 3 chunks of 64 channels (the edge layers' 21 / 42 / 85, vn2's 170), else all VN_CH (conv5, vn1)
#define URED_VN_BY_CHUNKS(LAUNCH)                                               \
    switch ((Co + 63) / 64) {                                                   \
        case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; \
        default: LAUNCH(VN_CH); break;                                          \
    }

int ured_vn_parts(int B, int N) {
    const long long BN = (long long)(B > 0 ? B : 0) * (N > 0 ? N : 0);
    const long long by_rows = (BN + URED_VN_STAT_ROWS - 1) / URED_VN_STAT_ROWS;
    return (int)(by_rows < URED_VN_PARTS ? (by_rows > 0 ? by_rows : 1) : URED_VN_PARTS);
}

int ured_vn_knn(const float* x, int B, int N, int D, int K, int* idx, float* ws, size_t ws_floats, void* stream) {
    ured::clear_error();
    URED_REQUIRE(B >= 0, "ured_vn_knn: negative size (B %d)", B);
    URED_REQUIRE(N >= 1, "ured_vn_knn: N %d must be at least 1", N);
    URED_REQUIRE(D >= 1 && D <= URED_VN_DMAX, "ured_vn_knn: D %d outside [1, %d]", D, URED_VN_DMAX);
    URED_REQUIRE(K >= 1 && K <= URED_VN_KMAX, "ured_vn_knn: K %d outside [1, %d]", K, URED_VN_KMAX);
    URED_REQUIRE(K <= N, "ured_vn_knn: K %d exceeds the cloud's %d points", K, N);
    URED_REQUIRE(B <= 65535 && (N + KN_T - 1) / KN_T <= 65535, "ured_vn_knn: B %d or N / 64 exceeds 65535", B);
    URED_REQUIRE((long long)B * N * (D > K ? D : K) < (1ll << 31), "ured_vn_knn: B * N * max(D, K) exceeds 2^31 - 1");
    const size_t need = (size_t)B * N * N;
    URED_REQUIRE(ws_floats >= need, "ured_vn_knn: workspace of %zu floats, %zu needed", ws_floats, need);
    if (B == 0) return 0;
    URED_REQUIRE(x && idx && ws, "ured_vn_knn: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int nt = (N + KN_T - 1) / KN_T;
    hipLaunchKernelGGL(vn_knn_dist_kernel, dim3(nt, nt, B), dim3(256), 0, st, x, N, D, ws);
    const int BN = B * N;
    hipLaunchKernelGGL(vn_knn_select_kernel, dim3((BN + VN_W - 1) / VN_W), dim3(VN_T), 0, st, ws, BN, N, K, idx);
    return ured::launch_status("ured_vn_knn");
}

int ured_vn_act_fwd(const float* uv, const int* idx, int B, int N, int k, int Co, int Cd, int training, const float* gamma,
                    const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked,
                    float momentum, float eps, int pool_mean, double* ws, size_t ws_doubles, float* stat, float* out,
                    unsigned char* mask, void* stream) {
    ured::clear_error();
    const bool edge = idx != nullptr;
    if (const int rc = vn_check("ured_vn_act_fwd", B, N, k, Co, Cd, edge)) return rc;
    URED_REQUIRE(!training || (long long)B * N * k > 1, "ured_vn_act_fwd: batch statistics need more than one value per channel");
    URED_REQUIRE(training || (running_mean && running_var), "ured_vn_act_fwd: eval needs the running statistics");
    const int parts = ured_vn_parts(B, N);
    URED_REQUIRE(!training || ws_doubles >= (size_t)parts * 2 * Co, "ured_vn_act_fwd: workspace of %zu doubles, %zu needed",
                 ws_doubles, (size_t)parts * 2 * Co);
    if (B == 0) return 0;
    URED_REQUIRE(uv && gamma && beta && stat && out && mask && (!training || ws), "ured_vn_act_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const VnShape s = vn_shape(B, N, k, Co, Cd, edge);
    const int rows = (s.BN + parts - 1) / parts;             // points per workgroup; parts * rows >= BN
    if (training)
        hipLaunchKernelGGL(vn_stat_fwd_kernel, dim3(parts, (Co + 63) / 64), dim3(VN_T), 0, st, uv, idx, s, rows, ws);
    hipLaunchKernelGGL(vn_stat_finalize_kernel, dim3((Co + VN_T - 1) / VN_T), dim3(VN_T), 0, st, training ? ws : nullptr, parts, Co,
                       (double)B * N * k, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, stat);
#define URED_VN_FWD(NN) hipLaunchKernelGGL(vn_act_fwd_kernel<NN>, dim3((s.BN + VN_W - 1) / VN_W), dim3(VN_T), 0, st, uv, idx, s, stat, pool_mean, out, mask)
    URED_VN_BY_CHUNKS(URED_VN_FWD)
#undef URED_VN_FWD
    return ured::launch_status("ured_vn_act_fwd");
}

int ured_vn_act_bwd(const float* grad_out, const float* uv, const int* idx, const unsigned char* mask, int B, int N, int k,
                    int Co, int Cd, int training, int pool_mean, const float* stat, double* ws, size_t ws_doubles, float* coef,
                    float* edge_ws, size_t edge_ws_floats, float* grad_uv, float* grad_gamma, float* grad_beta, void* stream) {
    ured::clear_error();
    const bool edge = idx != nullptr;
    if (const int rc = vn_check("ured_vn_act_bwd", B, N, k, Co, Cd, edge)) return rc;
    URED_REQUIRE((long long)N * k < (1ll << 31), "ured_vn_act_bwd: N * k exceeds 2^31 - 1");
    const int parts = ured_vn_parts(B, N);
    URED_REQUIRE(ws_doubles >= (size_t)parts * 2 * Co, "ured_vn_act_bwd: workspace of %zu doubles, %zu needed", ws_doubles,
                 (size_t)parts * 2 * Co);
    const size_t need = edge ? (size_t)B * N * k * 3 * (Co + Cd) : 0;
    URED_REQUIRE(edge_ws_floats >= need, "ured_vn_act_bwd: edge workspace of %zu floats, %zu needed", edge_ws_floats, need);
    URED_REQUIRE(grad_gamma && grad_beta && coef, "ured_vn_act_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {                                            // the sums over no edges
        if (hipMemsetAsync(grad_gamma, 0, sizeof(float) * Co, st) != hipSuccess ||
            hipMemsetAsync(grad_beta, 0, sizeof(float) * Co, st) != hipSuccess)
            return ured::launch_status("ured_vn_act_bwd");
        return 0;
    }
    URED_REQUIRE(grad_out && uv && mask && stat && ws && grad_uv && (!edge || edge_ws), "ured_vn_act_bwd: null pointer");
    const VnShape s = vn_shape(B, N, k, Co, Cd, edge);
    const int rows = (s.BN + parts - 1) / parts;
    hipLaunchKernelGGL(vn_stat_bwd_kernel, dim3(parts, (Co + 63) / 64), dim3(VN_T), 0, st, grad_out, uv, idx, mask, s, stat,
                       pool_mean, rows, ws);
    hipLaunchKernelGGL(vn_stat_bwd_finalize_kernel, dim3((Co + VN_T - 1) / VN_T), dim3(VN_T), 0, st, ws, parts, Co,
                       (double)B * N * k, training, grad_gamma, grad_beta, coef);
#define URED_VN_BWD(NN) hipLaunchKernelGGL(vn_act_bwd_kernel<NN>, dim3((s.BN + VN_W - 1) / VN_W), dim3(VN_T), 0, st, grad_out, uv, idx, mask, s, stat, coef, pool_mean, edge_ws, grad_uv)
    URED_VN_BY_CHUNKS(URED_VN_BWD)
#undef URED_VN_BWD
    if (edge)
        hipLaunchKernelGGL(vn_scatter_kernel, dim3((N + VN_P - 1) / VN_P, (3 * s.W + VN_C - 1) / VN_C, B), dim3(64), 0, st, edge_ws,
                           idx, N, k, s.W, s.LD, grad_uv);
    return ured::launch_status("ured_vn_act_bwd");
}

int ured_vn_maxpool_fwd(const float* x, const float* d, int B, int N, int k, int C, float* out, unsigned char* slot,
                        void* stream) {
    ured::clear_error();
    URED_REQUIRE(B >= 0 && N >= 1, "ured_vn_maxpool_fwd: negative size (B %d) or N %d below 1", B, N);
    URED_REQUIRE(k >= 1 && k <= URED_VN_KMAX, "ured_vn_maxpool_fwd: k %d outside [1, %d]", k, URED_VN_KMAX);
    if (const int rc = rows_check("ured_vn_maxpool_fwd", (long long)B * N * k, C)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(x && d && out && slot, "ured_vn_maxpool_fwd: null pointer");
    const long long total = (long long)B * N * C;
    hipLaunchKernelGGL(vn_maxpool_fwd_kernel, dim3((unsigned)((total + VN_T - 1) / VN_T)), dim3(VN_T), 0, (hipStream_t)stream, x, d,
                       k, C, (u32)total, out, slot);
    return ured::launch_status("ured_vn_maxpool_fwd");
}

int ured_vn_maxpool_bwd(const float* grad_out, const unsigned char* slot, int B, int N, int k, int C, float* grad_x,
                        void* stream) {
    ured::clear_error();
    URED_REQUIRE(B >= 0 && N >= 1, "ured_vn_maxpool_bwd: negative size (B %d) or N %d below 1", B, N);
    URED_REQUIRE(k >= 1 && k <= URED_VN_KMAX, "ured_vn_maxpool_bwd: k %d outside [1, %d]", k, URED_VN_KMAX);
    if (const int rc = rows_check("ured_vn_maxpool_bwd", (long long)B * N * k, C)) return rc;
    if (B == 0) return 0;
    URED_REQUIRE(grad_out && slot && grad_x, "ured_vn_maxpool_bwd: null pointer");
    const long long total = (long long)B * N * C;
    hipLaunchKernelGGL(vn_maxpool_bwd_kernel, dim3((unsigned)((total + VN_T - 1) / VN_T)), dim3(VN_T), 0, (hipStream_t)stream,
                       grad_out, slot, k, C, (u32)total, grad_x);
    return ured::launch_status("ured_vn_maxpool_bwd");
}

int ured_vn_frame_fwd(const float* x, const float* z, int rows, int C, float* out, void* stream) {
    ured::clear_error();
    if (const int rc = rows_check("ured_vn_frame_fwd", rows, C)) return rc;
    if (rows == 0) return 0;
    URED_REQUIRE(x && z && out, "ured_vn_frame_fwd: null pointer");
    const long long total = (long long)rows * C;
    hipLaunchKernelGGL(vn_frame_fwd_kernel, dim3((unsigned)((total + VN_T - 1) / VN_T)), dim3(VN_T), 0, (hipStream_t)stream, x, z, C,
                       (u32)total, out);
    return ured::launch_status("ured_vn_frame_fwd");
}

int ured_vn_frame_bwd(const float* grad_out, const float* x, const float* z, int rows, int C, float* grad_x, float* grad_z,
                      void* stream) {
    ured::clear_error();
    if (const int rc = rows_check("ured_vn_frame_bwd", rows, C)) return rc;
    if (rows == 0) return 0;
    URED_REQUIRE(grad_out && x && z && grad_x && grad_z, "ured_vn_frame_bwd: null pointer");
    hipLaunchKernelGGL(vn_frame_bwd_kernel, dim3((rows + VN_W - 1) / VN_W), dim3(VN_T), 0, (hipStream_t)stream, grad_out, x, z, rows,
                       C, grad_x, grad_z);
    return ured::launch_status("ured_vn_frame_bwd");
}

}  // extern "C"

URED_DBG_ACCESSOR(ured_dbg_vn)
