// The downstream STGODE predictor (reference model/STGODE/STGODE.py, odegcn.py; gpt-st_amd/predictors/stgode.py) on HIP.
// Activations are rows (b, t, n) x c, channels last, as for the other predictors.  A block of the model is BN_nodes(relu(step(relu(X)))):
// its temporal convolutions never run (predictors/stgode.py), and the ODE solve is one Euler step.
//
//   st_step_kernel     the step, forward and data backward, one launch over the whole batch and all frames.  With src = relu(In) (forward) or
//                      In (backward: In = g), per (b, tau) unit and node n
//                          Out[n, :] = cn oscale[n] (L (sscale . src))[n, :] + cw src[n, :] W + sum_k (ct M[tau][k] + [k = tau] cs) src[b, k, n, :]
//                      forward:  L = A,   oscale = alpha, W,   M = W2^T, cs = -11, relu on the way out; AT (kept for dalpha) = the bare node product
//                      backward: L = A^T, sscale = alpha (the SOURCE rows), W^T, M = W2, cs = -17 (x0 is detached), masked by [X > 0]
//                      A workgroup owns one unit and four 16-node tiles.  Per 32 channels: the unit's rows into the LDS slab, node_mix_slab
//                      (node_mix_dev.h) for the node product, then the channel product of the wave's 16 rows — held in registers for all c, W
//                      read from L2 (c x c <= 64 KB, the same for every workgroup; the slab leaves no LDS for it) — on the same MFMA, and
//                      the T-term time mix in the accumulator layout.  No product is written to memory but the one asked for (AT).
//   st_wgrad_kernel    dW^T = g^T relu(X): tap_wgrad_body (tap_wgrad_dev.h) with the relu in its source functor; row-split partials
//   st_reduce_kernel   dW2[k][m] = sum_{n, c} t[b, k, n, c] g[b, m, n, c] and dalpha[n] = sum_{tau, c} g AT per (b, node chunk): partials in a
//                      fixed order, summed by the caller
//   st_bn_*            batch norm with the NODE as the channel: statistics over the B T c values of a node.  Grid (N, S): split s owns a run
//                      of (b, t) rows.  stats: two passes per split (mean, then the squared deviations from it: nothing cancels), partial
//                      (mean, M2); apply: thread 0 folds the S partials in index order with Chan's update in double, then the split's rows are
//                      normalised — and, for the last block of a branch, folded into the running max over the branches (a later branch
//                      replaces where STRICTLY greater: exact ties stay with the lowest index).  Split 0 writes the saved statistics and
//                      updates the running ones as torch does (momentum, unbiased variance).  Backward: the two per-node sums as split
//                      partials, then dz and the relu mask of the step in one pass: g = dz [z > 0].
//
// fp32 MFMA 16x16x4 (exact fp32).  Plain launches only: no workgroup waits on another, nothing is accumulated with float atomics, the order of
// every sum is fixed.  No launch asks for more than the 64 KB of dynamic LDS a launch gets by default: N <= 448 (GPTST_ESHAPE beyond).
#include "common.h"
#include "gptst_hip.h"
#include "node_mix_dev.h"
#include "tap_wgrad_dev.h"

#define ST_MAX_NP 448       // 448 * NODE_MIX_P * 4 = 64 512 bytes of slab + the row of M: under 64 KB
#define ST_MAX_T 32
#define ST_MAX_C 128
#define ST_MAX_SPLIT 32
#define ST_RED_FLOATS 6144  // floats of t and of g a reduce workgroup holds: T (chunk c + 1) <= this

struct StStep {
    const float* L; int Np; const float* In; float* Out; float* AT; const float* W; const float* M; const float* oscale; const float* sscale;
    const float* mask; float cn, cw, ct, cs; int relu_in, relu_out, c, B, T, N;
};

__device__ __forceinline__ float4 st_relu4(float4 v) { return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)); }

__global__ __launch_bounds__(256) void st_step_kernel(StStep p) {
    extern __shared__ __attribute__((aligned(16))) float slab[];            // [Np][NODE_MIX_P]
    __shared__ float mrow[ST_MAX_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int unit = blockIdx.x, b = unit / p.T, tau = unit - b * p.T;
    const int n0 = (blockIdx.y * 4 + wave) * 16, c = p.c;
    const bool active = n0 < p.Np;
    if (tid < p.T) mrow[tid] = p.ct * p.M[tau * p.T + tid] + (tid == tau ? p.cs : 0.f);
    const size_t rbase = (size_t)unit * p.N;
    // the wave's 16 source rows for the channel product, all c channels: lane (j, kk) holds row n0 + j, columns 16 s + 4 kk .. + 3
    float4 treg[ST_MAX_C / 16];
    const bool rowok = active && n0 + j < p.N;
#pragma unroll
    for (int s = 0; s < ST_MAX_C / 16; ++s) {
        float4 v = f4zero();
        if (16 * s < c && rowok) v = ld4(p.In + (rbase + n0 + j) * c + 16 * s + 4 * kk);
        treg[s] = p.relu_in ? st_relu4(v) : v;
    }
    for (int cg = 0; cg * 32 < c; ++cg) {
        __syncthreads();                                                    // the previous group's reads of the slab are done (and mrow is written)
        for (int f = tid; f < p.Np * 8; f += 256) {
            const int m = f >> 3, c4 = f & 7;
            float4 v = f4zero();
            if (m < p.N && 32 * cg + 4 * c4 < c) {
                v = ld4(p.In + (rbase + m) * c + 32 * cg + 4 * c4);
                if (p.relu_in) v = st_relu4(v);
                if (p.sscale != nullptr) { const float a = p.sscale[m]; v = make_float4(a * v.x, a * v.y, a * v.z, a * v.w); }
            }
            st4(slab + m * NODE_MIX_P + 4 * c4, v);
        }
        __syncthreads();
        if (!active) continue;
        f32x4 acc[2], accw[2];
        acc[0] = acc[1] = accw[0] = accw[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        node_mix_slab(acc, p.L + (size_t)(n0 + j) * p.Np + 4 * kk, slab, p.Np, j, kk);
        const bool ct1 = 32 * cg + 16 < c;                                  // (wave-uniform: the second column tile exists)
#pragma unroll
        for (int s = 0; s < ST_MAX_C / 16; ++s) {
            if (16 * s >= c) break;
            const float tv[4] = {treg[s].x, treg[s].y, treg[s].z, treg[s].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float* wp = p.W + (size_t)(16 * s + 4 * kk + e) * c + 32 * cg + j;
                accw[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(tv[e], wp[0], accw[0], 0, 0, 0);
                if (ct1) accw[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(tv[e], wp[16], accw[1], 0, 0, 0);
            }
        }
        // ---- epilogue in the accumulator layout: reg r = (node n0 + kk*4 + r, channel 32 cg + 16 ct + j) ----
        // the time mix first, frame by frame: the eight loads of a frame are independent and in flight together (one element after the
        // other, a frame's load waits for the previous frame's: T dependent L2 latencies per element)
        const int nq = n0 + kk * 4;
        float tm[2][4];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) tm[ct][r] = 0.f;
#pragma unroll 2
        for (int k = 0; k < p.T; ++k) {
            const float mk = mrow[k];
            const float* src = p.In + (((size_t)b * p.T + k) * p.N + nq) * c + 32 * cg + j;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                if (ct == 1 && !ct1) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float s = nq + r < p.N ? src[(size_t)r * c + 16 * ct] : 0.f;
                    if (p.relu_in) s = fmaxf(s, 0.f);
                    tm[ct][r] = fmaf(mk, s, tm[ct][r]);
                }
            }
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int ch = 32 * cg + 16 * ct + j;
            if (32 * cg + 16 * ct >= c) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = nq + r;
                if (n >= p.N) continue;
                const size_t at = (rbase + n) * c + ch;
                const float a = acc[ct][r];
                if (p.AT != nullptr) p.AT[at] = a;
                float v = p.cn * (p.oscale != nullptr ? p.oscale[n] : 1.f) * a + p.cw * accw[ct][r] + tm[ct][r];
                if (p.relu_out) v = fmaxf(v, 0.f);
                if (p.mask != nullptr && !(p.mask[at] > 0.f)) v = 0.f;
                p.Out[at] = v;
            }
        }
    }
}

static inline bool st_shape_ok(int c, int T, int N) { return c >= 16 && c % 16 == 0 && c <= ST_MAX_C && T <= ST_MAX_T && 16 * ((N + 15) / 16) <= ST_MAX_NP; }

extern "C" int gptst_stgode_step(const float* L, int Np, const float* In, float* Out, float* AT, const float* W, const float* M, const float* oscale,
                                 const float* sscale, const float* mask, float cn, float cw, float ct, float cs, int relu_in, int relu_out, int c,
                                 int B, int T, int N, void* stream) {
    if (!L || !In || !Out || !W || !M || In == Out || B <= 0 || T <= 0 || N <= 0) return GPTST_EARG;
    if (!st_shape_ok(c, T, N) || Np != 16 * ((N + 15) / 16) || (long)B * T > 0x7fffffffL) return GPTST_ESHAPE;
    static_assert(ST_MAX_NP * NODE_MIX_P * sizeof(float) + ST_MAX_T * sizeof(float) <= 64 * 1024, "slab + the row of M exceed the default dynamic LDS");
    const size_t smem = (size_t)Np * NODE_MIX_P * sizeof(float);
    StStep p{L, Np, In, Out, AT, W, M, oscale, sscale, mask, cn, cw, ct, cs, relu_in, relu_out, c, B, T, N};
    hipLaunchKernelGGL(st_step_kernel, dim3((unsigned)(B * T), (Np / 16 + 3) / 4), dim3(256), smem, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

// ---- dW^T = g^T relu(X) ---------------------------------------------------------------------------------------------------------------------
struct StWgSrc {
    const float* X; int c, kcol;
    __device__ __forceinline__ float4 operator()(int row, bool rv) const {
        return (rv && kcol < c) ? st_relu4(ld4(X + (size_t)row * c + kcol)) : f4zero();
    }
};

__global__ __launch_bounds__(256) void st_wgrad_kernel(const float* G, const float* X, int c, float* part, int rows, int cps, int nchunks) {
    tap_wgrad_body(G, c, c, part, nullptr, rows, cps, nchunks, StWgSrc{X, c, (int)(blockIdx.x * 64 + 4 * (threadIdx.x & 15))});
}

extern "C" int gptst_stgode_wgrad_nsplit(int rows, int c) {
    if (rows <= 0 || c <= 0) return GPTST_EARG;
    return wgrad_split_rule(((c + 63) / 64) * ((c + 63) / 64), (rows + 63) / 64);
}

extern "C" int gptst_stgode_wgrad(const float* G, const float* X, int c, float* part, int nsplit, int rows, void* stream) {
    if (!G || !X || !part || rows <= 0) return GPTST_EARG;
    if (c < 16 || c % 16 || c > ST_MAX_C) return GPTST_ESHAPE;
    if (nsplit != gptst_stgode_wgrad_nsplit(rows, c)) return GPTST_EARG;
    const int nchunks = (rows + 63) / 64, cps = (nchunks + nsplit - 1) / nsplit;
    hipLaunchKernelGGL(st_wgrad_kernel, dim3((c + 63) / 64, (c + 63) / 64, nsplit), dim3(256), 0, (hipStream_t)stream, G, X, c, part, rows, cps, nchunks);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

// ---- block sums in a fixed order ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float st_block_sum(float v, float* red) {
    v = group_sum<64>(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float t = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return t;
}

// ---- dW2 and dalpha partials: grid (B, node chunks of nc nodes) -------------------------------------------------------------------------------
static inline int st_reduce_nc(int c, int T) { int nc = ST_RED_FLOATS / (T * (c + 1)); return nc < 1 ? 1 : nc > 8 ? 8 : nc; }

__global__ __launch_bounds__(256) void st_reduce_kernel(const float* G, const float* X, const float* AT, float* part2, float* parta, int c, int nc,
                                                        int T, int N) {
    __shared__ float tl[ST_RED_FLOATS + ST_MAX_T], gl[ST_RED_FLOATS + ST_MAX_T];          // [T][E + 1], E = (nodes of the chunk) * c
    __shared__ float red[4];
    const int tid = threadIdx.x, b = blockIdx.x, nb = blockIdx.y;
    const int n0 = nb * nc, nn = min(nc, N - n0), E = nn * c, P = nc * c + 1;
    for (int f = tid; f < T * E; f += 256) {
        const int k = f / E, e = f - k * E;
        const size_t at = (((size_t)b * T + k) * N + n0) * c + e;
        tl[k * P + e] = fmaxf(X[at], 0.f);
        gl[k * P + e] = G[at];
    }
    __syncthreads();
    for (int q = tid; q < T * T; q += 256) {
        const int k = q / T, m = q - k * T;
        float s = 0.f;
        for (int e = 0; e < E; ++e) s = fmaf(tl[k * P + e], gl[m * P + e], s);
        part2[((size_t)b * gridDim.y + nb) * T * T + q] = s;
    }
    for (int nl = 0; nl < nn; ++nl) {                                          // (nn is the same for every thread of the workgroup)
        float s = 0.f;
        for (int f = tid; f < T * c; f += 256) {
            const int k = f / c, ch = f - k * c;
            s = fmaf(gl[k * P + nl * c + ch], AT[(((size_t)b * T + k) * N + n0 + nl) * c + ch], s);
        }
        s = st_block_sum(s, red);
        if (tid == 0) parta[(size_t)b * N + n0 + nl] = s;
    }
}

extern "C" int gptst_stgode_reduce_nparts(int c, int T, int N) {
    if (c <= 0 || T <= 0 || N <= 0 || T > ST_MAX_T || c > ST_MAX_C) return GPTST_EARG;
    const int nc = st_reduce_nc(c, T);
    return (N + nc - 1) / nc;
}

extern "C" int gptst_stgode_reduce(const float* G, const float* X, const float* AT, float* part2, float* parta, int c, int B, int T, int N,
                                   void* stream) {
    if (!G || !X || !AT || !part2 || !parta || B <= 0 || T <= 0 || N <= 0) return GPTST_EARG;
    if (c < 16 || c % 16 || c > ST_MAX_C || T > ST_MAX_T || B > 65535) return GPTST_ESHAPE;
    const int nc = st_reduce_nc(c, T);
    static_assert(ST_MAX_T * (ST_MAX_C + 1) <= ST_RED_FLOATS + ST_MAX_T, "one node of the widest, longest shape exceeds the reduce tile");
    hipLaunchKernelGGL(st_reduce_kernel, dim3(B, (N + nc - 1) / nc), dim3(256), 0, (hipStream_t)stream, G, X, AT, part2, parta, c, nc, T, N);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

// ---- batch norm over the node channel ---------------------------------------------------------------------------------------------------------
// R = B T rows per node; split s owns the rows [s per, min(R, (s + 1) per)), per = ceil(R / S)
extern "C" int gptst_stgode_bn_nsplit(int R) {
    if (R <= 0) return GPTST_EARG;
    int S = (R + 31) / 32; if (S > ST_MAX_SPLIT) S = ST_MAX_SPLIT;
    const int per = (R + S - 1) / S;
    return (R + per - 1) / per;
}

struct StRows {
    int r0, r1, c4n;
    __device__ __forceinline__ StRows(int R, int S, int c) { const int per = (R + S - 1) / S; r0 = blockIdx.y * per; r1 = min(R, r0 + per); c4n = c >> 2; }
    __device__ __forceinline__ int count() const { return (r1 - r0) * c4n; }
    // float4 index f of the split -> offset of its first float: row r0 + f / c4n of node n
    __device__ __forceinline__ size_t at(int f, int n, int N) const { const int r = f / c4n; return ((size_t)(r0 + r) * N + n) * (4 * c4n) + 4 * (f - r * c4n); }
};

__global__ __launch_bounds__(256) void st_bn_stats_kernel(const float* Z, float* part, int c, int R, int N) {
    __shared__ float red[4];
    const int n = blockIdx.x, S = gridDim.y;
    const StRows rows(R, S, c);
    float s = 0.f;
    for (int f = threadIdx.x; f < rows.count(); f += 256) { const float4 v = ld4(Z + rows.at(f, n, N)); s += (v.x + v.y) + (v.z + v.w); }
    const float mean = st_block_sum(s, red) / (float)(4 * rows.count());
    float q = 0.f;
    for (int f = threadIdx.x; f < rows.count(); f += 256) {
        const float4 v = ld4(Z + rows.at(f, n, N));
        const float a = v.x - mean, b = v.y - mean, d = v.z - mean, e = v.w - mean;
        q += (a * a + b * b) + (d * d + e * e);
    }
    q = st_block_sum(q, red);
    if (threadIdx.x == 0) { part[((size_t)n * S + blockIdx.y) * 2] = mean; part[((size_t)n * S + blockIdx.y) * 2 + 1] = q; }
}

struct StBnApply {
    const float* Z; const float* part; const float* gamma; const float* beta; float* rmean; float* rvar; int training; float momentum, eps;
    float* Y; float* save_mean; float* save_rstd; float* best; int* which; int idx; int c, R, N;
};

__global__ __launch_bounds__(256) void st_bn_apply_kernel(StBnApply p) {
    __shared__ float st[2];
    const int n = blockIdx.x, S = gridDim.y;
    const StRows rows(p.R, S, p.c);
    if (threadIdx.x == 0) {
        float mean, rstd;
        if (p.part != nullptr) {                                               // Chan's update over the splits, in index order
            const int per = (p.R + S - 1) / S;
            double na = 0.0, mu = 0.0, m2 = 0.0;
            for (int s = 0; s < S; ++s) {
                const double nb = (double)(min(p.R, (s + 1) * per) - s * per) * p.c;
                const double mb = p.part[((size_t)n * S + s) * 2], qb = p.part[((size_t)n * S + s) * 2 + 1];
                const double d = mb - mu, nt = na + nb;
                mu += d * nb / nt;
                m2 += qb + d * d * na * nb / nt;
                na = nt;
            }
            mean = (float)mu;
            rstd = 1.f / sqrtf((float)(m2 / na) + p.eps);
            if (blockIdx.y == 0) {
                if (p.save_mean != nullptr) { p.save_mean[n] = mean; p.save_rstd[n] = rstd; }
                if (p.training && p.rmean != nullptr) {
                    p.rmean[n] = (1.f - p.momentum) * p.rmean[n] + p.momentum * mean;
                    p.rvar[n] = (1.f - p.momentum) * p.rvar[n] + p.momentum * (float)(m2 / (na > 1.0 ? na - 1.0 : 1.0));
                }
            }
        } else {
            mean = p.rmean[n];
            rstd = 1.f / sqrtf(p.rvar[n] + p.eps);
        }
        st[0] = mean; st[1] = rstd;
    }
    __syncthreads();
    const float mean = st[0], a = st[1] * p.gamma[n], bt = p.beta[n];
    for (int f = threadIdx.x; f < rows.count(); f += 256) {
        const size_t at = rows.at(f, n, p.N);
        const float4 z = ld4(p.Z + at);
        const float4 y = make_float4((z.x - mean) * a + bt, (z.y - mean) * a + bt, (z.z - mean) * a + bt, (z.w - mean) * a + bt);
        if (p.Y != nullptr) st4(p.Y + at, y);
        if (p.best != nullptr) {
            if (p.idx == 0) {
                st4(p.best + at, y);
                if (p.which != nullptr) *reinterpret_cast<int4*>(p.which + at) = make_int4(0, 0, 0, 0);
            } else {
                float4 o = ld4(p.best + at);
                const bool w0 = y.x > o.x, w1 = y.y > o.y, w2 = y.z > o.z, w3 = y.w > o.w;
                if (w0 || w1 || w2 || w3) {
                    if (w0) o.x = y.x;
                    if (w1) o.y = y.y;
                    if (w2) o.z = y.z;
                    if (w3) o.w = y.w;
                    st4(p.best + at, o);
                    if (p.which != nullptr) {
                        int4 wi = *reinterpret_cast<const int4*>(p.which + at);
                        if (w0) wi.x = p.idx;
                        if (w1) wi.y = p.idx;
                        if (w2) wi.z = p.idx;
                        if (w3) wi.w = p.idx;
                        *reinterpret_cast<int4*>(p.which + at) = wi;
                    }
                }
            }
        }
    }
}

extern "C" int gptst_stgode_bn_stats(const float* Z, float* part, int nsplit, int c, int B, int T, int N, void* stream) {
    if (!Z || !part || B <= 0 || T <= 0 || N <= 0 || (long)B * T > 0x7fffffffL / ST_MAX_C) return GPTST_EARG;
    if (c < 16 || c % 16 || c > ST_MAX_C || N > 65535 * 16) return GPTST_ESHAPE;
    if (nsplit != gptst_stgode_bn_nsplit(B * T)) return GPTST_EARG;
    hipLaunchKernelGGL(st_bn_stats_kernel, dim3(N, nsplit), dim3(256), 0, (hipStream_t)stream, Z, part, c, B * T, N);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_stgode_bn_apply(const float* Z, const float* part, int nsplit, const float* gamma, const float* beta, float* rmean, float* rvar,
                                     int training, float momentum, float eps, float* Y, float* save_mean, float* save_rstd, float* best, int* which,
                                     int idx, int c, int B, int T, int N, void* stream) {
    if (!Z || !gamma || !beta || (!Y && !best) || B <= 0 || T <= 0 || N <= 0 || idx < 0 || (long)B * T > 0x7fffffffL / ST_MAX_C) return GPTST_EARG;
    if ((part == nullptr && (!rmean || !rvar)) || (save_mean != nullptr) != (save_rstd != nullptr)) return GPTST_EARG;
    if (c < 16 || c % 16 || c > ST_MAX_C) return GPTST_ESHAPE;
    if (nsplit != gptst_stgode_bn_nsplit(B * T)) return GPTST_EARG;
    StBnApply p{Z, part, gamma, beta, rmean, rvar, training, momentum, eps, Y, save_mean, save_rstd, best, which, idx, c, B * T, N};
    hipLaunchKernelGGL(st_bn_apply_kernel, dim3(N, nsplit), dim3(256), 0, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

// backward: dy = dY, or dBest where this branch (idx) holds the max
struct StBnBwd {
    const float* dY; const float* dBest; const int* which; int idx; const float* Z; const float* gamma; const float* mean; const float* rstd;
    float* part; float* G; float* dgamma; float* dbeta; int c, R, N;
};

__device__ __forceinline__ float4 st_dy(const StBnBwd& p, size_t at) {
    if (p.dY != nullptr) return ld4(p.dY + at);
    const float4 d = ld4(p.dBest + at);
    const int4 w = *reinterpret_cast<const int4*>(p.which + at);
    return make_float4(w.x == p.idx ? d.x : 0.f, w.y == p.idx ? d.y : 0.f, w.z == p.idx ? d.z : 0.f, w.w == p.idx ? d.w : 0.f);
}

__global__ __launch_bounds__(256) void st_bn_bwd_reduce_kernel(StBnBwd p) {
    __shared__ float red[4];
    const int n = blockIdx.x, S = gridDim.y;
    const StRows rows(p.R, S, p.c);
    const float mean = p.mean[n], rstd = p.rstd[n];
    float s1 = 0.f, s2 = 0.f;
    for (int f = threadIdx.x; f < rows.count(); f += 256) {
        const size_t at = rows.at(f, n, p.N);
        const float4 d = st_dy(p, at), z = ld4(p.Z + at);
        s1 += (d.x + d.y) + (d.z + d.w);
        s2 += (d.x * ((z.x - mean) * rstd) + d.y * ((z.y - mean) * rstd)) + (d.z * ((z.z - mean) * rstd) + d.w * ((z.w - mean) * rstd));
    }
    s1 = st_block_sum(s1, red);
    s2 = st_block_sum(s2, red);
    if (threadIdx.x == 0) { p.part[((size_t)n * S + blockIdx.y) * 2] = s1; p.part[((size_t)n * S + blockIdx.y) * 2 + 1] = s2; }
}

__global__ __launch_bounds__(256) void st_bn_bwd_apply_kernel(StBnBwd p) {
    __shared__ float st[2];
    const int n = blockIdx.x, S = gridDim.y;
    const StRows rows(p.R, S, p.c);
    if (threadIdx.x == 0) {
        double s1 = 0.0, s2 = 0.0;
        for (int s = 0; s < S; ++s) { s1 += p.part[((size_t)n * S + s) * 2]; s2 += p.part[((size_t)n * S + s) * 2 + 1]; }
        if (blockIdx.y == 0) { p.dbeta[n] = (float)s1; p.dgamma[n] = (float)s2; }
        const double cnt = (double)p.R * p.c;
        st[0] = (float)(s1 / cnt); st[1] = (float)(s2 / cnt);
    }
    __syncthreads();
    const float m1 = st[0], m2 = st[1], mean = p.mean[n], rstd = p.rstd[n], a = p.gamma[n] * rstd;
    for (int f = threadIdx.x; f < rows.count(); f += 256) {
        const size_t at = rows.at(f, n, p.N);
        const float4 d = st_dy(p, at), z = ld4(p.Z + at);
        float4 g;
        g.x = z.x > 0.f ? a * (d.x - m1 - (z.x - mean) * rstd * m2) : 0.f;
        g.y = z.y > 0.f ? a * (d.y - m1 - (z.y - mean) * rstd * m2) : 0.f;
        g.z = z.z > 0.f ? a * (d.z - m1 - (z.z - mean) * rstd * m2) : 0.f;
        g.w = z.w > 0.f ? a * (d.w - m1 - (z.w - mean) * rstd * m2) : 0.f;
        st4(p.G + at, g);
    }
}

extern "C" int gptst_stgode_bn_bwd(const float* dY, const float* dBest, const int* which, int idx, const float* Z, const float* gamma,
                                   const float* mean, const float* rstd, float* part, int nsplit, float* G, float* dgamma, float* dbeta, int c,
                                   int B, int T, int N, int stage, void* stream) {
    if (!Z || !gamma || !mean || !rstd || !part || B <= 0 || T <= 0 || N <= 0 || (long)B * T > 0x7fffffffL / ST_MAX_C) return GPTST_EARG;
    if ((dY == nullptr) == (dBest == nullptr) || (dBest != nullptr && !which) || (stage != 0 && stage != 1)) return GPTST_EARG;
    if (stage == 1 && (!G || !dgamma || !dbeta)) return GPTST_EARG;
    if (c < 16 || c % 16 || c > ST_MAX_C) return GPTST_ESHAPE;
    if (nsplit != gptst_stgode_bn_nsplit(B * T)) return GPTST_EARG;
    StBnBwd p{dY, dBest, which, idx, Z, gamma, mean, rstd, part, G, dgamma, dbeta, c, B * T, N};
    if (stage == 0) hipLaunchKernelGGL(st_bn_bwd_reduce_kernel, dim3(N, nsplit), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(st_bn_bwd_apply_kernel, dim3(N, nsplit), dim3(256), 0, (hipStream_t)stream, p);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}
