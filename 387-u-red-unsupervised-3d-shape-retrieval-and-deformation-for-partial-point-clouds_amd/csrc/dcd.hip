// dcd.hip — density-aware chamfer as a training loss for MI355X / gfx950.
//
// Replaces the torch tail of calc_dcd under autograd
//   Density_aware_Chamfer_Distance/utils_v2/model_utils.py:13-51
// (exp, scatter_add_, gather, pow, mean and their autograd, ~a dozen launch-bound elementwise
// ops each way) by one reduction kernel forward and one gather kernel backward.
//
// Forward (ured_dcd_loss_fwd): the arithmetic and the fixed-order reductions of dcd_kernel
//   (csrc/nn.hip), one workgroup per item, NN visit counts in LDS by integer atomics (exact).
//   The exponent is a float. Besides the loss it stores, per point, the derivative of the
//   item's loss with respect to that point's squared distance (the weights are detached, as in
//   the reference: model_utils.py:35,41):
//     coef1[j] = alpha exp(-alpha d1[j]) w1[j] / (2 n1),   coef2 likewise.
// Backward (ured_dcd_loss_bwd): ONE launch for both point gradients. The per-point distance
//   gradient g_loss[b] coef[j] + gd[j] is formed in the kernel and goes through the gather-form
//   backward of nn_bwd_kernel (csrc/nn.hip): own term first, then the other side's entries in
//   ascending index, ballot compaction per wave, no float atomics, every output written with '='.
#define URED_DBG_FILE 16
#include "ured_common.h"
#include "../../include/ured_hip.h"

namespace {

constexpr int DCD_THREADS = 256;
constexpr int DCD_MAX_POINTS = 16384;   // n1 + n2 per item (64 KiB of LDS counts)
constexpr int DCD_TILE = 1024;          // other-side entries per LDS tile of the backward

// count^lambda; mode 0: 1, 1: c, 2: c*c, 3: sqrtf(c), 4: powf(c, lambda)
__device__ __forceinline__ float count_pow(int c, int mode, float lam) {
    const float f = (float)c;
    switch (mode) {
        case 0: return 1.0f;
        case 1: return f;
        case 2: return f * f;
        case 3: return sqrtf(f);
        default: return powf(f, lam);
    }
}

__global__ __launch_bounds__(DCD_THREADS) void dcd_loss_fwd_kernel(
        const float* __restrict__ d1, const int* __restrict__ i1, const float* __restrict__ d2,
        const int* __restrict__ i2, int n1, int n2, float alpha, float lam, int mode, float frac12, float frac21,
        float* __restrict__ loss, float* __restrict__ cdp, float* __restrict__ cdt, float* __restrict__ coef1,
        float* __restrict__ coef2) {
    extern __shared__ int cnt[];            // [n2] visits of x points by gt NNs, then [n1] vice versa
    __shared__ float red[6][DCD_THREADS];
    int* c1 = cnt;                           // indexed by idx1 (an x point)
    int* c2 = cnt + n2;                      // indexed by idx2 (a gt point)
    const int b = blockIdx.x, t = threadIdx.x;
    const float* D1 = d1 + (size_t)b * n1; const int* I1 = i1 + (size_t)b * n1;
    const float* D2 = d2 + (size_t)b * n2; const int* I2 = i2 + (size_t)b * n2;
    for (int k = t; k < n1 + n2; k += DCD_THREADS) cnt[k] = 0;
    __syncthreads();
    for (int k = t; k < n1; k += DCD_THREADS) {
        const int id = I1[k];
        URED_DBG_CHECK((unsigned)id < (unsigned)n2);     // LDS counter index
        atomicAdd(&c1[id], 1);
    }
    for (int k = t; k < n2; k += DCD_THREADS) {
        const int id = I2[k];
        URED_DBG_CHECK((unsigned)id < (unsigned)n1);
        atomicAdd(&c2[id], 1);
    }
    __syncthreads();
    const float fn1 = (float)n1, fn2 = (float)n2;
    float l1 = 0.f, l2 = 0.f, s1 = 0.f, s2 = 0.f, t1 = 0.f, t2 = 0.f;
    for (int k = t; k < n1; k += DCD_THREADS) {
        const float d = D1[k];
        const float w = (1.0f / (count_pow(c1[I1[k]], mode, lam) + 1e-6f)) * frac21;
        const float ew = expf(-d * alpha) * w;
        l1 += 1.0f - ew;
        s1 += sqrtf(d);
        t1 += d;
        if (coef1) coef1[(size_t)b * n1 + k] = alpha * ew / (2.0f * fn1);
    }
    for (int k = t; k < n2; k += DCD_THREADS) {
        const float d = D2[k];
        const float w = (1.0f / (count_pow(c2[I2[k]], mode, lam) + 1e-6f)) * frac12;
        const float ew = expf(-d * alpha) * w;
        l2 += 1.0f - ew;
        s2 += sqrtf(d);
        t2 += d;
        if (coef2) coef2[(size_t)b * n2 + k] = alpha * ew / (2.0f * fn2);
    }
    red[0][t] = l1; red[1][t] = l2; red[2][t] = s1; red[3][t] = s2; red[4][t] = t1; red[5][t] = t2;
    __syncthreads();
    for (int h = DCD_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int q = 0; q < 6; ++q) red[q][t] += red[q][t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        loss[b] = (red[0][0] / fn1 + red[1][0] / fn2) / 2.0f;
        if (cdp) cdp[b] = (red[2][0] / fn1 + red[3][0] / fn2) / 2.0f;
        if (cdt) cdt[b] = red[4][0] / fn1 + red[5][0] / fn2;
    }
}

struct DcdBwdArgs {
    const float* xyz1; const float* xyz2;    // gt [b,n1,3], x [b,n2,3]
    const int* idx1; const int* idx2;
    const float* coef1; const float* coef2;
    const float* g_loss;                     // [b] or nullptr (no gradient through the loss)
    const float* gd1; const float* gd2;      // further gradients of dist1 / dist2, or nullptr
    int n1, n2;
    float* g1; float* g2;                    // nullptr: that side is skipped
};

// Gradient for the points of one side of an item (blockIdx.z 0: the gt points, 1: the x points).
__global__ __launch_bounds__(DCD_THREADS) void dcd_loss_bwd_kernel(DcdBwdArgs args) {
    __shared__ __attribute__((aligned(16))) int sidx[DCD_TILE];
    __shared__ float sg[DCD_TILE], sx[DCD_TILE], sy[DCD_TILE], sz[DCD_TILE];
    __shared__ int slist[(DCD_THREADS / 64) * DCD_TILE];   // per-wave compacted entry lists
    const int dir = blockIdx.z, s = blockIdx.y;
    const float *P, *O, *cfP, *cfO, *gdP, *gdO; const int *idxP, *idxO; float* gP; int p_len, o_len;
    if (dir == 0) { P = args.xyz1; O = args.xyz2; cfP = args.coef1; cfO = args.coef2; gdP = args.gd1; gdO = args.gd2;
                    idxP = args.idx1; idxO = args.idx2; gP = args.g1; p_len = args.n1; o_len = args.n2; }
    else          { P = args.xyz2; O = args.xyz1; cfP = args.coef2; cfO = args.coef1; gdP = args.gd2; gdO = args.gd1;
                    idxP = args.idx2; idxO = args.idx1; gP = args.g2; p_len = args.n2; o_len = args.n1; }
    if (!gP) return;                         // uniform per block
    const int j0 = blockIdx.x * DCD_THREADS;
    if (j0 >= p_len) return;
    const size_t p_off = (size_t)s * p_len, o_off = (size_t)s * o_len;
    const bool has_l = args.g_loss != nullptr;
    const float gl = has_l ? args.g_loss[s] : 0.f;
    const int j = j0 + threadIdx.x;
    const bool valid = j < p_len;
    const int jc = valid ? j : p_len - 1;
    const float* pj = P + 3 * (p_off + jc);
    const float px = pj[0], py = pj[1], pz = pj[2];
    float ax = 0.f, ay = 0.f, az = 0.f;
    if (has_l || gdP) {
        const int id = idxP[p_off + jc];
        URED_DBG_CHECK((unsigned)id < (unsigned)o_len);   // the NN index lies in the other side
        const float* r = O + 3 * (o_off + id);
        float gj = has_l ? gl * cfP[p_off + jc] : 0.f;
        if (gdP) gj += gdP[p_off + jc];
        const float g = gj * 2.f;
        ax = g * (px - r[0]); ay = g * (py - r[1]); az = g * (pz - r[2]);
    }
    if (has_l || gdO) {
        for (int t0 = 0; t0 < o_len; t0 += DCD_TILE) {
            const int tn = min(DCD_TILE, o_len - t0);
            __syncthreads();
            for (int i = threadIdx.x; i < DCD_TILE; i += DCD_THREADS) {
                int id = -1; float gg = 0.f, x = 0.f, y = 0.f, z = 0.f;
                if (i < tn) {
                    const size_t k = o_off + t0 + i;
                    id = idxO[k];
                    gg = has_l ? gl * cfO[k] : 0.f;
                    if (gdO) gg += gdO[k];
                    x = O[3 * k]; y = O[3 * k + 1]; z = O[3 * k + 2];
                }
                sidx[i] = id; sg[i] = gg; sx[i] = x; sy[i] = y; sz[i] = z;
            }
            __syncthreads();
            // Each wave compacts, in ascending k, the tile entries whose NN lands in its own 64
            // points (ballot + prefix popcount), then walks only that list; the owner lane
            // accumulates: own term first, then k ascending, as a full ascending scan would.
            const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
            const int jw0 = j0 + wv * 64;
            int* lst = slist + wv * DCD_TILE;
            int cnt = 0;
            for (int c = 0; c < tn; c += 64) {
                const int k = c + ln;
                const int id = k < tn ? sidx[k] : -1;
                const bool pred = (unsigned)(id - jw0) < 64u;
                const unsigned long long mask = __ballot(pred);
                if (pred) lst[cnt + __popcll(mask & ((1ull << ln) - 1ull))] = k;
                cnt += __popcll(mask);
            }
            for (int e = 0; e < cnt; ++e) {
                const int k = lst[e];
                const bool own = sidx[k] == j;
                const float g = sg[k] * 2.f;
                const float nx = ax - g * (sx[k] - px);
                const float ny = ay - g * (sy[k] - py);
                const float nz = az - g * (sz[k] - pz);
                ax = own ? nx : ax; ay = own ? ny : ay; az = own ? nz : az;
            }
        }
    }
    if (valid) {
        float* o = gP + 3 * (p_off + j);
        o[0] = ax; o[1] = ay; o[2] = az;
    }
}

}  // namespace

extern "C" {

int ured_dcd_loss_fwd(const float* dist1, const int* idx1, const float* dist2, const int* idx2, int b, int n1, int n2,
                      float alpha, float lambda, float frac_12, float frac_21, float* loss, float* cd_p, float* cd_t,
                      float* coef1, float* coef2, void* stream) {
    ured::clear_error();
    URED_REQUIRE(b >= 0 && n1 > 0 && n2 > 0, "ured_dcd_loss_fwd: bad sizes b=%d n1=%d n2=%d", b, n1, n2);
    URED_REQUIRE(n1 + n2 <= DCD_MAX_POINTS, "ured_dcd_loss_fwd: n1+n2=%d exceeds %d", n1 + n2, DCD_MAX_POINTS);
    URED_REQUIRE(lambda >= 0.f, "ured_dcd_loss_fwd: lambda must be >= 0");
    if (b == 0) return 0;
    URED_REQUIRE(dist1 && idx1 && dist2 && idx2 && loss, "ured_dcd_loss_fwd: null pointer");
    const int mode = lambda == 0.f ? 0 : lambda == 1.f ? 1 : lambda == 2.f ? 2 : lambda == 0.5f ? 3 : 4;
    hipLaunchKernelGGL(dcd_loss_fwd_kernel, dim3(b), dim3(DCD_THREADS), (size_t)(n1 + n2) * sizeof(int),
                       (hipStream_t)stream, dist1, idx1, dist2, idx2, n1, n2, alpha, lambda, mode, frac_12, frac_21,
                       loss, cd_p, cd_t, coef1, coef2);
    return ured::launch_status("ured_dcd_loss_fwd");
}

int ured_dcd_loss_bwd(const float* xyz1, const float* xyz2, const int* idx1, const int* idx2, const float* coef1,
                      const float* coef2, const float* g_loss, const float* gd1, const float* gd2, int b, int n1,
                      int n2, float* gxyz1, float* gxyz2, void* stream) {
    ured::clear_error();
    URED_REQUIRE(b >= 0 && n1 > 0 && n2 > 0, "ured_dcd_loss_bwd: bad sizes b=%d n1=%d n2=%d", b, n1, n2);
    URED_REQUIRE(b <= 65535, "ured_dcd_loss_bwd: b %d exceeds 65535", b);
    if (b == 0 || (!gxyz1 && !gxyz2)) return 0;
    URED_REQUIRE(xyz1 && xyz2 && idx1 && idx2, "ured_dcd_loss_bwd: null pointer");
    URED_REQUIRE(!g_loss || (coef1 && coef2), "ured_dcd_loss_bwd: g_loss needs coef1 and coef2");
    DcdBwdArgs a{xyz1, xyz2, idx1, idx2, coef1, coef2, g_loss, gd1, gd2, n1, n2, gxyz1, gxyz2};
    const int max_p = n1 > n2 ? n1 : n2;
    hipLaunchKernelGGL(dcd_loss_bwd_kernel, dim3((max_p + DCD_THREADS - 1) / DCD_THREADS, b, 2), dim3(DCD_THREADS), 0,
                       (hipStream_t)stream, a);
    return ured::launch_status("ured_dcd_loss_bwd");
}

}  // extern "C"

URED_DBG_ACCESSOR(ured_dbg_dcd)
