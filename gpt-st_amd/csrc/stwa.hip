// One cut of a Layer of the downstream ST-WA predictor (reference model/ST_WA/ST_WA.py:138-164, attention.py; gpt-st_amd/predictors/stwa.py)
// on HIP, forward and backward.  C channels (16 or 32), 8 heads of HS = C / 8.  A cut attends from 2 proxy rows over 2 + R rows of one node
// (temporal), then over the N nodes of one sample (spatial).  Its four linear maps have per-(sample, node) weights that an MLP generates:
//
//     F_g(x) = x W_g(b, n) + bias_g(b, n),    W_g = V[g][0] + sum_k co[b, n, g, k] V[g][1 + k],    bias_g = u[g][0] + sum_k cb[b, n, g, k] u[g][1 + k]
//
// (g = 0 temporal key, 1 temporal value, 2 spatial key, 3 spatial value).  The generated weight is rank 5 in (b, n): a thread that owns output
// channel j of a node folds its column of W_g from V (6 C loads that every node shares, from L1 / L2) into registers and applies it to that
// node's rows, so no (B, N, C, C) tensor exists anywhere, and the N x N scores of the spatial attention are recomputed from K and V of the
// sample, which sit in LDS (2 proxies x (K, V) x N x C floats), and never leave the workgroup.
//
//   local fwd     grid (node tiles, B)   rows = [prox + out_{i-1} | data rows];  Kt, Vt = F_0, F_1(rows);  softmax over the 2 + R keys per (node,
//                                         proxy, head);  T = tp2(tanh(tp1(.)));  Ks, Vs = F_2, F_3(T)  ->  T, Ks, Vs (B, 2, N, C)
//   spatial fwd   grid (query tiles, B)  Ks, Vs of the sample -> LDS;  softmax over the N keys per (query node, proxy, head), two passes, a fixed
//                                         order;  U = sp2(relu(sp1(.)));  g = sigmoid(ag2(relu(ag1(U))));  out_i = sum_p g U -> slot i of Y;
//                                         kept when asked: the mixed values S and each row's maximum and sum
//   spatial bwd q grid (query tiles, B)  the tail backwards from S (recomputed, not stored), dS, D = <dS, S>, and the query side of the
//                                         attention: dT;  the tail's weight gradients into the workgroup's slab
//   spatial bwd kv grid (key tiles, B)   T, dS, D, max, sum of the sample -> LDS;  a thread owns (key node, proxy, head) and sweeps the queries in
//                                         index order: dKs, dVs with no sum across workgroups
//   local bwd     grid (node tiles, B)   recomputes the forward of its tile, then F_2, F_3, tp2, tp1, the temporal attention, F_0, F_1 backwards:
//                                         dh rows, the proxies' gradient per sample, the gradient carried to cut i - 1 through out_{i-1}, dco, dcb
//                                         (each (b, n) has one owner: added across the cut launches), dV, du and the two Linears' gradients into
//                                         the workgroup's slab
//
// Weight gradients: a workgroup (b, tile) owns one slab of gptst_stwa_slab_floats(C) floats and adds into it across the cut launches of a layer
// (every entry has one owning thread; the launches are ordered by the stream); the caller sums the slabs once per layer.  No float atomics: a
// repeated run is bit-identical.  Plain launches only: no workgroup waits on another.
#include "common.h"
#include "gptst_hip.h"
#include <algorithm>
#include "recur_step_dev.h"      // recur_launch: the launch with the dynamic-LDS attribute above 64 KB

#define SW_TN 16                 // nodes per workgroup
#define SW_RC 8                  // row capacity of the temporal arrays: 2 proxies + at most 6 data rows
#define SW_HEADS 8
#define SW_NT RECUR_THREADS      // 256 = SW_TN nodes x 2 proxies x 8 heads
// the keys of a node: unrolled to the capacity and guarded, so that arrays indexed by the key stay in registers
#define SW_KEYS(m, n) _Pragma("unroll") for (int m = 0; m < SW_RC; ++m) if (m < (n))

enum { SW_TP1 = 0, SW_TP2 = 1, SW_SP1 = 2, SW_SP2 = 3, SW_AG1 = 4, SW_AG2 = 5 };
enum { SW_ACT_NONE = 0, SW_ACT_RELU = 1, SW_ACT_TANH = 2, SW_ACT_SIGMOID = 3 };

struct SwArgs {
    int B, T, N, cuts, cut, cs, R;                     // R = data rows of this cut: clamp(T - cut cs, 0, cs)
    const float *h, *prox, *co, *cb, *V, *u;           // h (B, T, N, C); prox (2 cuts, N, C); co, cb (B, N, 4, 5); V (4, 6, C, C); u (4, 6, C)
    const float *Wl, *WlT, *bl;                        // the six shared Linears [out][in], their transposes [in][out], biases (6, C)
    float* Y;                                          // (B, cuts, N, C): slot cut - 1 read by local, slot cut written by spatial fwd
    float *Tq, *Ks, *Vs;                               // (B, 2, N, C)
    float *S, *mx, *sm;                                // (B, 2, N, C), (B, 2, N, 8) x 2: kept for the backward (NULL: not written)
    const float *dY, *carry_in;                        // dY (B, cuts, N, C); the gradient of out_i that cut i + 1 handed back (B, N, C) or NULL
    float *dS, *Dq, *dTq, *dKs, *dVs;                  // (B, 2, N, C); Dq (B, 2, N, 8)
    float *dh, *dPb, *carry_out, *dco, *dcb, *slab;    // dh (B, T, N, C) | NULL; dPb (B, 2 cuts, N, C) | NULL; carry (B, N, C) | NULL; slab | NULL
};

template <int C> struct SwSlab {                       // one workgroup's weight-gradient partials, in floats
    static constexpr int V = 0, U = 24 * C * C, W = U + 24 * C, Bl = W + 6 * C * C, SIZE = Bl + 6 * C;
};

template <int ACT> __device__ __forceinline__ float sw_act(float x) {
    if (ACT == SW_ACT_RELU) return x > 0.f ? x : 0.f;
    if (ACT == SW_ACT_TANH) return tanhf(x);
    if (ACT == SW_ACT_SIGMOID) return sigmoidf_(x);
    return x;
}

// ---- row phases: an item is (node n of the tile, channel); rows of a node lie [n][cap][C] in LDS ----------------------------------------
// cw, cbv [n][4][6] in LDS: (1, co[b, n, g, :]) and (1, cb[b, n, g, :])
template <int C>
__device__ void sw_load_coef(const SwArgs& p, int b, int n0, int nv, float* cw, float* cbv) {
    for (int it = threadIdx.x; it < nv * 24; it += SW_NT) {
        const int n = it / 24, g = (it / 6) % 4, k = it % 6;
        float a = 1.f, c = 1.f;
        if (k > 0) {
            const size_t o = (((size_t)b * p.N + n0 + n) * 4 + g) * 5 + (k - 1);
            a = p.co[o];
            c = p.cb[o];
        }
        cw[it] = a;
        cbv[it] = c;
    }
}

// dst[n][m][j] = F_g(src[n][m])_j for m < rows
template <int C>
__device__ void sw_gen_fwd(const SwArgs& p, int g, const float* cw, const float* cbv, const float* src, int scap, int rows, float* dst, int dcap,
                           int nv) {
    for (int it = threadIdx.x; it < SW_TN * C; it += SW_NT) {
        const int n = it / C, j = it % C;
        if (n >= nv) continue;
        const float *cn = cw + (n * 4 + g) * 6, *bn = cbv + (n * 4 + g) * 6;
        float wc[C], be = 0.f;
#pragma unroll
        for (int i = 0; i < C; ++i) {
            float w = 0.f;
#pragma unroll
            for (int k = 0; k < 6; ++k) w = fmaf(cn[k], p.V[((size_t)(g * 6 + k) * C + i) * C + j], w);
            wc[i] = w;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) be = fmaf(bn[k], p.u[(g * 6 + k) * C + j], be);
        for (int m = 0; m < rows; ++m) {
            const float* x = src + (n * scap + m) * C;
            float acc = be;
#pragma unroll
            for (int i = 0; i < C; ++i) acc = fmaf(x[i], wc[i], acc);
            dst[(n * dcap + m) * C + j] = acc;
        }
    }
}

// dx[n][m][i] (+)= sum_j W_g[i][j] dout[n][m][j]
template <int C>
__device__ void sw_gen_bwd_x(const SwArgs& p, int g, const float* cw, const float* dout, int ocap, int rows, float* dx, int xcap, bool add, int nv) {
    for (int it = threadIdx.x; it < SW_TN * C; it += SW_NT) {
        const int n = it / C, i = it % C;
        if (n >= nv) continue;
        const float* cn = cw + (n * 4 + g) * 6;
        float wr[C];
#pragma unroll
        for (int j = 0; j < C; ++j) {
            float w = 0.f;
#pragma unroll
            for (int k = 0; k < 6; ++k) w = fmaf(cn[k], p.V[((size_t)(g * 6 + k) * C + i) * C + j], w);
            wr[j] = w;
        }
        for (int m = 0; m < rows; ++m) {
            const float* d = dout + (n * ocap + m) * C;
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < C; ++j) acc = fmaf(d[j], wr[j], acc);
            float* o = dx + (n * xcap + m) * C + i;
            *o = add ? *o + acc : acc;
        }
    }
}

// dco[b, n, g, k] += sum_ij V[g][1 + k][i][j] sum_m x[m][i] dout[m][j];  dcb[b, n, g, k] += sum_j u[g][1 + k][j] sum_m dout[m][j]  (bias: the
// temporal key's bias is common to all keys of a query and cancels in the softmax: its gradient is exactly 0 and is left there)
template <int C>
__device__ void sw_gen_bwd_coef(const SwArgs& p, int g, bool bias, const float* src, int scap, const float* dout, int ocap, int rows, int b, int n0,
                                int nv) {
    for (int it = threadIdx.x; it < SW_TN * C; it += SW_NT) {              // (no early exit: the C lanes of a node reduce by shuffles)
        const int n = it / C, j = it % C;
        const bool valid = n < nv;
        float dw[C], sd = 0.f;
#pragma unroll
        for (int i = 0; i < C; ++i) dw[i] = 0.f;
        if (valid)
            for (int m = 0; m < rows; ++m) {
                const float d = dout[(n * ocap + m) * C + j];
                const float* x = src + (n * scap + m) * C;
                sd += d;
#pragma unroll
                for (int i = 0; i < C; ++i) dw[i] = fmaf(x[i], d, dw[i]);
            }
        for (int k = 1; k < 6; ++k) {
            float pk = 0.f;
#pragma unroll
            for (int i = 0; i < C; ++i) pk = fmaf(p.V[((size_t)(g * 6 + k) * C + i) * C + j], dw[i], pk);
            float qk = p.u[(g * 6 + k) * C + j] * sd;
#pragma unroll
            for (int o = C / 2; o > 0; o >>= 1) {
                pk += __shfl_xor(pk, o);
                qk += __shfl_xor(qk, o);
            }
            if (valid && j == 0) {
                const size_t o = (((size_t)b * p.N + n0 + n) * 4 + g) * 5 + (k - 1);
                p.dco[o] += pk;
                if (bias) p.dcb[o] += qk;
            }
        }
    }
}

// the slab's dV[g][k][i][j] += sum_n cw[n][g][k] sum_m x[n][m][i] dout[n][m][j];  du[g][k][j] += sum_n cbv[n][g][k] sum_m dout[n][m][j]
template <int C>
__device__ void sw_gen_bwd_w(int g, bool bias, const float* cw, const float* cbv, const float* src, int scap, const float* dout, int ocap, int rows,
                             float* slab, int nv) {
    for (int e = threadIdx.x; e < C * C; e += SW_NT) {
        const int i = e / C, j = e % C;
        float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int n = 0; n < nv; ++n) {
            float dw = 0.f;
            for (int m = 0; m < rows; ++m) dw = fmaf(src[(n * scap + m) * C + i], dout[(n * ocap + m) * C + j], dw);
#pragma unroll
            for (int k = 0; k < 6; ++k) acc[k] = fmaf(cw[(n * 4 + g) * 6 + k], dw, acc[k]);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) slab[SwSlab<C>::V + (g * 6 + k) * C * C + e] += acc[k];
    }
    if (!bias) return;
    for (int e = threadIdx.x; e < 6 * C; e += SW_NT) {
        const int k = e / C, j = e % C;
        float acc = 0.f;
        for (int n = 0; n < nv; ++n) {
            float sd = 0.f;
            for (int m = 0; m < rows; ++m) sd += dout[(n * ocap + m) * C + j];
            acc = fmaf(cbv[(n * 4 + g) * 6 + k], sd, acc);
        }
        slab[SwSlab<C>::U + (g * 6 + k) * C + j] += acc;
    }
}

// the shared Linears on the 2 proxy rows of a node, arrays [n][2][C]:  dst = act(src W_l^T + b_l)
template <int C, int ACT>
__device__ void sw_lin_fwd(const SwArgs& p, int l, const float* src, float* dst, int nv) {
    for (int it = threadIdx.x; it < SW_TN * C; it += SW_NT) {
        const int n = it / C, j = it % C;
        if (n >= nv) continue;
        const float* wt = p.WlT + (size_t)l * C * C;
        float a0 = p.bl[l * C + j], a1 = a0;
        const float *x0 = src + (n * 2) * C, *x1 = x0 + C;
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const float w = wt[i * C + j];
            a0 = fmaf(x0[i], w, a0);
            a1 = fmaf(x1[i], w, a1);
        }
        dst[(n * 2) * C + j] = sw_act<ACT>(a0);
        dst[(n * 2 + 1) * C + j] = sw_act<ACT>(a1);
    }
}

// dx (+)= dy W_l, then times the derivative of the activation that PRODUCED x, from its output y (ACT of the layer below; NONE: no factor)
template <int C, int ACT>
__device__ void sw_lin_bwd_x(const SwArgs& p, int l, const float* dy, float* dx, bool add, const float* y, int nv) {
    for (int it = threadIdx.x; it < SW_TN * C; it += SW_NT) {
        const int n = it / C, i = it % C;
        if (n >= nv) continue;
        const float* w = p.Wl + (size_t)l * C * C;
        float a0 = 0.f, a1 = 0.f;
        const float *d0 = dy + (n * 2) * C, *d1 = d0 + C;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const float wv = w[j * C + i];
            a0 = fmaf(d0[j], wv, a0);
            a1 = fmaf(d1[j], wv, a1);
        }
        float* o = dx + (n * 2) * C + i;
        if (add) { a0 += o[0]; a1 += o[C]; }
        if (ACT == SW_ACT_RELU) { a0 = y[(n * 2) * C + i] > 0.f ? a0 : 0.f; a1 = y[(n * 2 + 1) * C + i] > 0.f ? a1 : 0.f; }
        if (ACT == SW_ACT_TANH) { const float y0 = y[(n * 2) * C + i], y1 = y[(n * 2 + 1) * C + i]; a0 *= 1.f - y0 * y0; a1 *= 1.f - y1 * y1; }
        o[0] = a0;
        o[C] = a1;
    }
}

// the slab's dW_l[j][i] += sum_n sum_m dy[n][m][j] x[n][m][i];  db_l[j] += sum_n sum_m dy[n][m][j]
template <int C>
__device__ void sw_lin_bwd_w(int l, const float* dy, const float* x, float* slab, int nv) {
    for (int e = threadIdx.x; e < C * C; e += SW_NT) {
        const int j = e / C, i = e % C;
        float acc = 0.f;
        for (int n = 0; n < nv; ++n) {
            acc = fmaf(dy[(n * 2) * C + j], x[(n * 2) * C + i], acc);
            acc = fmaf(dy[(n * 2 + 1) * C + j], x[(n * 2 + 1) * C + i], acc);
        }
        slab[SwSlab<C>::W + l * C * C + e] += acc;
    }
    for (int j = threadIdx.x; j < C; j += SW_NT) {
        float acc = 0.f;
        for (int n = 0; n < nv; ++n) acc += dy[(n * 2) * C + j] + dy[(n * 2 + 1) * C + j];
        slab[SwSlab<C>::Bl + l * C + j] += acc;
    }
}

// ---- the node-local half ------------------------------------------------------------------------------------------------------------------
template <int C> struct SwLocal {                      // LDS carve of the two local kernels, in floats
    static constexpr int BIG = SW_TN * SW_RC * C, SMALL = SW_TN * 2 * C, COEF = SW_TN * 24;
    static constexpr int FWD = 3 * BIG + 3 * SMALL + 2 * COEF, BWD = 6 * BIG + 9 * SMALL + 2 * COEF;
};

// rows, Kt, Vt, O, H1, T of the tile (what local fwd computes and local bwd recomputes)
template <int C>
__device__ void sw_local_body(const SwArgs& p, int b, int n0, int nv, const float* cw, const float* cbv, float* rows, float* Kt, float* Vt, float* O,
                              float* H1, float* Tt) {
    constexpr int HS = C / SW_HEADS;
    const int R2 = 2 + p.R, tid = threadIdx.x;
    for (int it = tid; it < nv * R2 * C; it += SW_NT) {
        const int n = it / (R2 * C), m = (it / C) % R2, c = it % C;
        float v;
        if (m < 2) {
            v = p.prox[((size_t)(2 * p.cut + m) * p.N + n0 + n) * C + c];
            if (p.cut > 0) v += p.Y[(((size_t)b * p.cuts + p.cut - 1) * p.N + n0 + n) * C + c];
        } else {
            v = p.h[(((size_t)b * p.T + p.cut * p.cs + m - 2) * p.N + n0 + n) * C + c];
        }
        rows[(n * SW_RC + m) * C + c] = v;
    }
    __syncthreads();
    sw_gen_fwd<C>(p, 0, cw, cbv, rows, SW_RC, R2, Kt, SW_RC, nv);
    sw_gen_fwd<C>(p, 1, cw, cbv, rows, SW_RC, R2, Vt, SW_RC, nv);
    __syncthreads();
    {
        const int n = tid / 16, pp = (tid / 8) % 2, hd = tid % 8;
        if (n < nv) {
            const float scale = 1.f / sqrtf((float)HS);
            const float* q = rows + (n * SW_RC + pp) * C + hd * HS;
            float s[SW_RC], mxv = -INFINITY, l = 0.f, o[HS];
            SW_KEYS(m, R2) {
                const float* k = Kt + (n * SW_RC + m) * C + hd * HS;
                float d = 0.f;
#pragma unroll
                for (int e = 0; e < HS; ++e) d = fmaf(q[e], k[e], d);
                s[m] = d * scale;
                mxv = fmaxf(mxv, s[m]);
            }
#pragma unroll
            for (int e = 0; e < HS; ++e) o[e] = 0.f;
            SW_KEYS(m, R2) {
                const float a = expf(s[m] - mxv);
                const float* v = Vt + (n * SW_RC + m) * C + hd * HS;
                l += a;
#pragma unroll
                for (int e = 0; e < HS; ++e) o[e] = fmaf(a, v[e], o[e]);
            }
#pragma unroll
            for (int e = 0; e < HS; ++e) O[(n * 2 + pp) * C + hd * HS + e] = o[e] / l;
        }
    }
    __syncthreads();
    sw_lin_fwd<C, SW_ACT_TANH>(p, SW_TP1, O, H1, nv);
    __syncthreads();
    sw_lin_fwd<C, SW_ACT_NONE>(p, SW_TP2, H1, Tt, nv);
    __syncthreads();
}

template <int C>
__global__ __launch_bounds__(SW_NT) void sw_local_fwd_kernel(SwArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    using L = SwLocal<C>;
    float *rows = smem, *Kt = rows + L::BIG, *Vt = Kt + L::BIG, *O = Vt + L::BIG, *H1 = O + L::SMALL, *Tt = H1 + L::SMALL;
    float *cw = Tt + L::SMALL, *cbv = cw + L::COEF;
    const int b = blockIdx.y, n0 = blockIdx.x * SW_TN, nv = min(SW_TN, p.N - n0);
    sw_load_coef<C>(p, b, n0, nv, cw, cbv);
    __syncthreads();
    sw_local_body<C>(p, b, n0, nv, cw, cbv, rows, Kt, Vt, O, H1, Tt);
    sw_gen_fwd<C>(p, 2, cw, cbv, Tt, 2, 2, Kt, 2, nv);                    // Ks, Vs over the temporal arrays: those are done with
    sw_gen_fwd<C>(p, 3, cw, cbv, Tt, 2, 2, Vt, 2, nv);
    __syncthreads();
    for (int it = threadIdx.x; it < nv * 2 * C; it += SW_NT) {
        const int n = it / (2 * C), pp = (it / C) % 2, c = it % C;
        const size_t o = (((size_t)b * 2 + pp) * p.N + n0 + n) * C + c;
        p.Tq[o] = Tt[it];
        p.Ks[o] = Kt[it];
        p.Vs[o] = Vt[it];
    }
}

template <int C>
__global__ __launch_bounds__(SW_NT) void sw_local_bwd_kernel(SwArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    using L = SwLocal<C>;
    constexpr int HS = C / SW_HEADS;
    float *rows = smem, *Kt = rows + L::BIG, *Vt = Kt + L::BIG, *dKt = Vt + L::BIG, *dVt = dKt + L::BIG, *dR = dVt + L::BIG;
    float *O = dR + L::BIG, *H1 = O + L::SMALL, *Tt = H1 + L::SMALL, *dT = Tt + L::SMALL, *dH = dT + L::SMALL, *dO = dH + L::SMALL;
    float *dKs = dO + L::SMALL, *dVs = dKs + L::SMALL, *dP = dVs + L::SMALL, *cw = dP + L::SMALL, *cbv = cw + L::COEF;
    const int tid = threadIdx.x, b = blockIdx.y, n0 = blockIdx.x * SW_TN, nv = min(SW_TN, p.N - n0), R2 = 2 + p.R;
    float* slab = p.slab ? p.slab + ((size_t)b * gridDim.x + blockIdx.x) * SwSlab<C>::SIZE : nullptr;
    sw_load_coef<C>(p, b, n0, nv, cw, cbv);
    for (int it = tid; it < nv * 2 * C; it += SW_NT) {
        const int n = it / (2 * C), pp = (it / C) % 2, c = it % C;
        const size_t o = (((size_t)b * 2 + pp) * p.N + n0 + n) * C + c;
        dT[it] = p.dTq[o];
        dKs[it] = p.dKs[o];
        dVs[it] = p.dVs[o];
    }
    __syncthreads();
    sw_local_body<C>(p, b, n0, nv, cw, cbv, rows, Kt, Vt, O, H1, Tt);

    // Ks = F_2(T), Vs = F_3(T), and T is the spatial query
    sw_gen_bwd_x<C>(p, 2, cw, dKs, 2, 2, dT, 2, true, nv);
    __syncthreads();
    sw_gen_bwd_x<C>(p, 3, cw, dVs, 2, 2, dT, 2, true, nv);
    sw_gen_bwd_coef<C>(p, 2, true, Tt, 2, dKs, 2, 2, b, n0, nv);
    sw_gen_bwd_coef<C>(p, 3, true, Tt, 2, dVs, 2, 2, b, n0, nv);
    if (slab) {
        sw_gen_bwd_w<C>(2, true, cw, cbv, Tt, 2, dKs, 2, 2, slab, nv);
        sw_gen_bwd_w<C>(3, true, cw, cbv, Tt, 2, dVs, 2, 2, slab, nv);
    }
    __syncthreads();
    // T = tp2(H1), H1 = tanh(tp1(O))
    sw_lin_bwd_x<C, SW_ACT_TANH>(p, SW_TP2, dT, dH, false, H1, nv);
    __syncthreads();
    sw_lin_bwd_x<C, SW_ACT_NONE>(p, SW_TP1, dH, dO, false, nullptr, nv);
    if (slab) {
        sw_lin_bwd_w<C>(SW_TP2, dT, H1, slab, nv);
        sw_lin_bwd_w<C>(SW_TP1, dH, O, slab, nv);
    }
    __syncthreads();
    // the temporal attention: a thread owns (node, head) and both proxies, so that dKt, dVt of a key have one writer
    if (tid < SW_TN * SW_HEADS) {
        const int n = tid / SW_HEADS, hd = tid % SW_HEADS;
        if (n < nv) {
            const float scale = 1.f / sqrtf((float)HS);
            float dk[SW_RC][HS], dv[SW_RC][HS];
            SW_KEYS(m, R2)
#pragma unroll
                for (int e = 0; e < HS; ++e) dk[m][e] = dv[m][e] = 0.f;
            for (int pp = 0; pp < 2; ++pp) {
                const float* q = rows + (n * SW_RC + pp) * C + hd * HS;
                const float* go = dO + (n * 2 + pp) * C + hd * HS;
                float a[SW_RC], da[SW_RC], mxv = -INFINITY, l = 0.f, dd = 0.f, dq[HS];
                SW_KEYS(m, R2) {
                    const float* k = Kt + (n * SW_RC + m) * C + hd * HS;
                    float d = 0.f;
#pragma unroll
                    for (int e = 0; e < HS; ++e) d = fmaf(q[e], k[e], d);
                    a[m] = d * scale;
                    mxv = fmaxf(mxv, a[m]);
                }
                SW_KEYS(m, R2) {
                    a[m] = expf(a[m] - mxv);
                    l += a[m];
                }
                SW_KEYS(m, R2) {
                    const float* v = Vt + (n * SW_RC + m) * C + hd * HS;
                    float d = 0.f;
#pragma unroll
                    for (int e = 0; e < HS; ++e) d = fmaf(go[e], v[e], d);
                    a[m] /= l;
                    da[m] = d;
                    dd = fmaf(a[m], d, dd);
                }
#pragma unroll
                for (int e = 0; e < HS; ++e) dq[e] = 0.f;
                SW_KEYS(m, R2) {
                    const float ds = a[m] * (da[m] - dd) * scale;
                    const float* k = Kt + (n * SW_RC + m) * C + hd * HS;
#pragma unroll
                    for (int e = 0; e < HS; ++e) {
                        dq[e] = fmaf(ds, k[e], dq[e]);
                        dk[m][e] = fmaf(ds, q[e], dk[m][e]);
                        dv[m][e] = fmaf(a[m], go[e], dv[m][e]);
                    }
                }
#pragma unroll
                for (int e = 0; e < HS; ++e) dP[(n * 2 + pp) * C + hd * HS + e] = dq[e];
            }
            SW_KEYS(m, R2)
#pragma unroll
                for (int e = 0; e < HS; ++e) {
                    dKt[(n * SW_RC + m) * C + hd * HS + e] = dk[m][e];
                    dVt[(n * SW_RC + m) * C + hd * HS + e] = dv[m][e];
                }
        }
    }
    __syncthreads();
    // Kt = F_0(rows), Vt = F_1(rows)
    sw_gen_bwd_x<C>(p, 0, cw, dKt, SW_RC, R2, dR, SW_RC, false, nv);
    __syncthreads();
    sw_gen_bwd_x<C>(p, 1, cw, dVt, SW_RC, R2, dR, SW_RC, true, nv);
    sw_gen_bwd_coef<C>(p, 0, false, rows, SW_RC, dKt, SW_RC, R2, b, n0, nv);
    sw_gen_bwd_coef<C>(p, 1, true, rows, SW_RC, dVt, SW_RC, R2, b, n0, nv);
    if (slab) {
        sw_gen_bwd_w<C>(0, false, cw, cbv, rows, SW_RC, dKt, SW_RC, R2, slab, nv);
        sw_gen_bwd_w<C>(1, true, cw, cbv, rows, SW_RC, dVt, SW_RC, R2, slab, nv);
    }
    __syncthreads();
    // the proxy rows are queries and keys: their gradient goes to the proxies (per sample) and, summed over both, back through out_{i-1}
    for (int it = tid; it < nv * C; it += SW_NT) {
        const int n = it / C, c = it % C;
        const float t0 = dR[(n * SW_RC) * C + c] + dP[(n * 2) * C + c], t1 = dR[(n * SW_RC + 1) * C + c] + dP[(n * 2 + 1) * C + c];
        if (p.dPb) {
            p.dPb[(((size_t)b * 2 * p.cuts + 2 * p.cut) * p.N + n0 + n) * C + c] = t0;
            p.dPb[(((size_t)b * 2 * p.cuts + 2 * p.cut + 1) * p.N + n0 + n) * C + c] = t1;
        }
        if (p.carry_out) p.carry_out[((size_t)b * p.N + n0 + n) * C + c] = t0 + t1;
    }
    if (p.dh)
        for (int it = tid; it < nv * p.R * C; it += SW_NT) {
            const int n = it / (p.R * C), r = (it / C) % p.R, c = it % C;
            p.dh[(((size_t)b * p.T + p.cut * p.cs + r) * p.N + n0 + n) * C + c] = dR[(n * SW_RC + 2 + r) * C + c];
        }
}

// ---- the spatial half -----------------------------------------------------------------------------------------------------------------------
template <int C> struct SwSpatial {                    // LDS in floats: [2][N][C] arrays of the sample, then [SW_TN][2][C] arrays of the tile
    static constexpr int SMALL = SW_TN * 2 * C;
    static size_t fwd(int N) { return (size_t)4 * N * C + 6 * SMALL; }
    static size_t bwd_q(int N) { return (size_t)4 * N * C + 11 * SMALL; }
    static size_t bwd_kv(int N) { return (size_t)4 * N * C + (size_t)3 * 2 * N * SW_HEADS; }
};

// n floats (a multiple of 4, both sides 16-byte aligned) from global memory into LDS
__device__ __forceinline__ void sw_stage(float* dst, const float* src, int n) {
    for (int i = 4 * threadIdx.x; i < n; i += 4 * SW_NT) st4(dst + i, ld4(src + i));
}

template <int C>
__device__ void sw_load_tile(float* dst, const float* src, int b, int n0, int nv, int N) {
    for (int it = threadIdx.x; it < nv * 2 * C; it += SW_NT) {
        const int n = it / (2 * C), pp = (it / C) % 2, c = it % C;
        dst[it] = src[(((size_t)b * 2 + pp) * N + n0 + n) * C + c];
    }
}

// the tail from the mixed values: G1 = relu(sp1(S)), U = sp2(G1), A1 = relu(ag1(U)), Gt = sigmoid(ag2(A1))
template <int C>
__device__ void sw_tail_fwd(const SwArgs& p, const float* S, float* G1, float* U, float* A1, float* Gt, int nv) {
    sw_lin_fwd<C, SW_ACT_RELU>(p, SW_SP1, S, G1, nv);
    __syncthreads();
    sw_lin_fwd<C, SW_ACT_NONE>(p, SW_SP2, G1, U, nv);
    __syncthreads();
    sw_lin_fwd<C, SW_ACT_RELU>(p, SW_AG1, U, A1, nv);
    __syncthreads();
    sw_lin_fwd<C, SW_ACT_SIGMOID>(p, SW_AG2, A1, Gt, nv);
    __syncthreads();
}

template <int C>
__global__ __launch_bounds__(SW_NT) void sw_spatial_fwd_kernel(SwArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int HS = C / SW_HEADS, SM = SwSpatial<C>::SMALL;
    const int N = p.N, tid = threadIdx.x, b = blockIdx.y, n0 = blockIdx.x * SW_TN, nv = min(SW_TN, N - n0);
    float *Kl = smem, *Vl = Kl + (size_t)2 * N * C, *Q = Vl + (size_t)2 * N * C, *S = Q + SM, *G1 = S + SM, *U = G1 + SM, *A1 = U + SM, *Gt = A1 + SM;
    sw_stage(Kl, p.Ks + (size_t)b * 2 * N * C, 2 * N * C);
    sw_stage(Vl, p.Vs + (size_t)b * 2 * N * C, 2 * N * C);
    sw_load_tile<C>(Q, p.Tq, b, n0, nv, N);
    __syncthreads();
    {
        const int n = tid / 16, pp = (tid / 8) % 2, hd = tid % 8;
        if (n < nv) {
            const float scale = 1.f / sqrtf((float)HS);
            float q[HS], o[HS], mxv = -INFINITY, l = 0.f;
#pragma unroll
            for (int e = 0; e < HS; ++e) { q[e] = Q[(n * 2 + pp) * C + hd * HS + e]; o[e] = 0.f; }
            const float *kb = Kl + (size_t)pp * N * C + hd * HS, *vb = Vl + (size_t)pp * N * C + hd * HS;
            for (int m = 0; m < N; ++m) {
                float d = 0.f;
#pragma unroll
                for (int e = 0; e < HS; ++e) d = fmaf(q[e], kb[m * C + e], d);
                mxv = fmaxf(mxv, d * scale);
            }
            for (int m = 0; m < N; ++m) {
                float d = 0.f;
#pragma unroll
                for (int e = 0; e < HS; ++e) d = fmaf(q[e], kb[m * C + e], d);
                const float a = expf(d * scale - mxv);
                l += a;
#pragma unroll
                for (int e = 0; e < HS; ++e) o[e] = fmaf(a, vb[m * C + e], o[e]);
            }
            const size_t row = ((size_t)b * 2 + pp) * N + n0 + n;
#pragma unroll
            for (int e = 0; e < HS; ++e) {
                const float v = o[e] / l;
                S[(n * 2 + pp) * C + hd * HS + e] = v;
                if (p.S) p.S[row * C + hd * HS + e] = v;
            }
            if (p.mx) {
                p.mx[row * SW_HEADS + hd] = mxv;
                p.sm[row * SW_HEADS + hd] = l;
            }
        }
    }
    __syncthreads();
    sw_tail_fwd<C>(p, S, G1, U, A1, Gt, nv);
    for (int it = tid; it < nv * C; it += SW_NT) {
        const int n = it / C, c = it % C;
        p.Y[(((size_t)b * p.cuts + p.cut) * N + n0 + n) * C + c] =
            Gt[(n * 2) * C + c] * U[(n * 2) * C + c] + Gt[(n * 2 + 1) * C + c] * U[(n * 2 + 1) * C + c];
    }
}

template <int C>
__global__ __launch_bounds__(SW_NT) void sw_spatial_bwd_q_kernel(SwArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int HS = C / SW_HEADS, SM = SwSpatial<C>::SMALL;
    const int N = p.N, tid = threadIdx.x, b = blockIdx.y, n0 = blockIdx.x * SW_TN, nv = min(SW_TN, N - n0);
    float *Kl = smem, *Vl = Kl + (size_t)2 * N * C, *Q = Vl + (size_t)2 * N * C, *S = Q + SM, *G1 = S + SM, *U = G1 + SM, *A1 = U + SM, *Gt = A1 + SM;
    float *dU = Gt + SM, *dG = dU + SM, *dA = dG + SM, *dZ = dA + SM, *dSl = dZ + SM;
    float* slab = p.slab ? p.slab + ((size_t)b * gridDim.x + blockIdx.x) * SwSlab<C>::SIZE : nullptr;
    sw_stage(Kl, p.Ks + (size_t)b * 2 * N * C, 2 * N * C);
    sw_stage(Vl, p.Vs + (size_t)b * 2 * N * C, 2 * N * C);
    sw_load_tile<C>(Q, p.Tq, b, n0, nv, N);
    sw_load_tile<C>(S, p.S, b, n0, nv, N);
    __syncthreads();
    sw_tail_fwd<C>(p, S, G1, U, A1, Gt, nv);
    for (int it = tid; it < nv * 2 * C; it += SW_NT) {                    // out = sum_p g U
        const int n = it / (2 * C), c = it % C;
        float d = p.dY[(((size_t)b * p.cuts + p.cut) * N + n0 + n) * C + c];
        if (p.carry_in) d += p.carry_in[((size_t)b * N + n0 + n) * C + c];
        const float g = Gt[it];
        dZ[it] = d * U[it] * g * (1.f - g);
        dU[it] = d * g;
    }
    __syncthreads();
    sw_lin_bwd_x<C, SW_ACT_RELU>(p, SW_AG2, dZ, dA, false, A1, nv);
    __syncthreads();
    sw_lin_bwd_x<C, SW_ACT_NONE>(p, SW_AG1, dA, dU, true, nullptr, nv);
    __syncthreads();
    sw_lin_bwd_x<C, SW_ACT_RELU>(p, SW_SP2, dU, dG, false, G1, nv);
    __syncthreads();
    sw_lin_bwd_x<C, SW_ACT_NONE>(p, SW_SP1, dG, dSl, false, nullptr, nv);
    if (slab) {
        sw_lin_bwd_w<C>(SW_AG2, dZ, A1, slab, nv);
        sw_lin_bwd_w<C>(SW_AG1, dA, U, slab, nv);
        sw_lin_bwd_w<C>(SW_SP2, dU, G1, slab, nv);
        sw_lin_bwd_w<C>(SW_SP1, dG, S, slab, nv);
    }
    __syncthreads();
    {
        const int n = tid / 16, pp = (tid / 8) % 2, hd = tid % 8;
        if (n < nv) {
            const float scale = 1.f / sqrtf((float)HS);
            const size_t row = ((size_t)b * 2 + pp) * N + n0 + n;
            const float mxv = p.mx[row * SW_HEADS + hd], l = p.sm[row * SW_HEADS + hd];
            float q[HS], ds[HS], dq[HS], dd = 0.f;
#pragma unroll
            for (int e = 0; e < HS; ++e) {
                const int o = (n * 2 + pp) * C + hd * HS + e;
                q[e] = Q[o];
                ds[e] = dSl[o];
                dq[e] = 0.f;
                dd = fmaf(ds[e], S[o], dd);
                p.dS[row * C + hd * HS + e] = ds[e];
            }
            p.Dq[row * SW_HEADS + hd] = dd;
            const float *kb = Kl + (size_t)pp * N * C + hd * HS, *vb = Vl + (size_t)pp * N * C + hd * HS;
            for (int m = 0; m < N; ++m) {
                float d = 0.f, dp = 0.f;
#pragma unroll
                for (int e = 0; e < HS; ++e) {
                    d = fmaf(q[e], kb[m * C + e], d);
                    dp = fmaf(ds[e], vb[m * C + e], dp);
                }
                const float dsc = expf(d * scale - mxv) / l * (dp - dd) * scale;
#pragma unroll
                for (int e = 0; e < HS; ++e) dq[e] = fmaf(dsc, kb[m * C + e], dq[e]);
            }
#pragma unroll
            for (int e = 0; e < HS; ++e) p.dTq[row * C + hd * HS + e] = dq[e];
        }
    }
}

template <int C>
__global__ __launch_bounds__(SW_NT) void sw_spatial_bwd_kv_kernel(SwArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int HS = C / SW_HEADS;
    const int N = p.N, tid = threadIdx.x, b = blockIdx.y, n0 = blockIdx.x * SW_TN, nv = min(SW_TN, N - n0);
    float *Ql = smem, *Gl = Ql + (size_t)2 * N * C, *Ml = Gl + (size_t)2 * N * C, *Ll = Ml + 2 * N * SW_HEADS, *Dl = Ll + 2 * N * SW_HEADS;
    sw_stage(Ql, p.Tq + (size_t)b * 2 * N * C, 2 * N * C);
    sw_stage(Gl, p.dS + (size_t)b * 2 * N * C, 2 * N * C);
    sw_stage(Ml, p.mx + (size_t)b * 2 * N * SW_HEADS, 2 * N * SW_HEADS);
    sw_stage(Ll, p.sm + (size_t)b * 2 * N * SW_HEADS, 2 * N * SW_HEADS);
    sw_stage(Dl, p.Dq + (size_t)b * 2 * N * SW_HEADS, 2 * N * SW_HEADS);
    __syncthreads();
    const int n = tid / 16, pp = (tid / 8) % 2, hd = tid % 8;
    if (n >= nv) return;
    const float scale = 1.f / sqrtf((float)HS);
    const size_t row = ((size_t)b * 2 + pp) * N + n0 + n;
    float k[HS], v[HS], dk[HS], dv[HS];
#pragma unroll
    for (int e = 0; e < HS; ++e) {
        k[e] = p.Ks[row * C + hd * HS + e];
        v[e] = p.Vs[row * C + hd * HS + e];
        dk[e] = dv[e] = 0.f;
    }
    const float *qb = Ql + (size_t)pp * N * C + hd * HS, *gb = Gl + (size_t)pp * N * C + hd * HS;
    const float *mb = Ml + pp * N * SW_HEADS + hd, *lb = Ll + pp * N * SW_HEADS + hd, *db = Dl + pp * N * SW_HEADS + hd;
    for (int m = 0; m < N; ++m) {                                          // the queries, in index order
        float d = 0.f, dp = 0.f;
#pragma unroll
        for (int e = 0; e < HS; ++e) {
            d = fmaf(qb[m * C + e], k[e], d);
            dp = fmaf(gb[m * C + e], v[e], dp);
        }
        const float a = expf(d * scale - mb[m * SW_HEADS]) / lb[m * SW_HEADS];
        const float dsc = a * (dp - db[m * SW_HEADS]) * scale;
#pragma unroll
        for (int e = 0; e < HS; ++e) {
            dk[e] = fmaf(dsc, qb[m * C + e], dk[e]);
            dv[e] = fmaf(a, gb[m * C + e], dv[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < HS; ++e) {
        p.dKs[row * C + hd * HS + e] = dk[e];
        p.dVs[row * C + hd * HS + e] = dv[e];
    }
}

// ---- launch ---------------------------------------------------------------------------------------------------------------------------------
enum { SW_K_LOCAL_FWD, SW_K_SPATIAL_FWD, SW_K_BWD_Q, SW_K_BWD_KV, SW_K_LOCAL_BWD };

template <int C>
static size_t sw_lds(int kernel, int N) {
    switch (kernel) {
        case SW_K_LOCAL_FWD: return sizeof(float) * SwLocal<C>::FWD;
        case SW_K_LOCAL_BWD: return sizeof(float) * SwLocal<C>::BWD;
        case SW_K_SPATIAL_FWD: return sizeof(float) * SwSpatial<C>::fwd(N);
        case SW_K_BWD_Q: return sizeof(float) * SwSpatial<C>::bwd_q(N);
        default: return sizeof(float) * SwSpatial<C>::bwd_kv(N);
    }
}

static size_t sw_lds_any(int kernel, int N, int C) { return C == 16 ? sw_lds<16>(kernel, N) : sw_lds<32>(kernel, N); }

static int sw_check(const SwArgs& p, int C, bool temporal) {
    if (p.B <= 0 || p.B > 65535 || p.N <= 0 || p.cuts <= 0 || p.cut < 0 || p.cut >= p.cuts) return GPTST_EARG;
    if (temporal && (p.T <= 0 || p.cs <= 0)) return GPTST_EARG;
    if ((C != 16 && C != 32) || (temporal && p.cs > SW_RC - 2)) return GPTST_ESHAPE;
    return GPTST_OK;
}

template <int K, int C>
static int sw_launch_c(const SwArgs& p, hipStream_t stream) {
    const size_t smem = sw_lds<C>(K, p.N);
    if (smem > RECUR_LDS_MAX) return GPTST_ESHAPE;
    const dim3 grid((p.N + SW_TN - 1) / SW_TN, p.B);
    if (K == SW_K_LOCAL_FWD) return recur_launch<sw_local_fwd_kernel<C>>(p, grid, smem, stream);
    if (K == SW_K_SPATIAL_FWD) return recur_launch<sw_spatial_fwd_kernel<C>>(p, grid, smem, stream);
    if (K == SW_K_BWD_Q) return recur_launch<sw_spatial_bwd_q_kernel<C>>(p, grid, smem, stream);
    if (K == SW_K_BWD_KV) return recur_launch<sw_spatial_bwd_kv_kernel<C>>(p, grid, smem, stream);
    return recur_launch<sw_local_bwd_kernel<C>>(p, grid, smem, stream);
}

template <int K>
static int sw_launch(SwArgs p, int C, bool temporal, void* stream) {
    const int rc = sw_check(p, C, temporal);
    if (rc != GPTST_OK) return rc;
    if (temporal) p.R = std::max(0, std::min(p.cs, p.T - p.cut * p.cs));
    return C == 16 ? sw_launch_c<K, 16>(p, (hipStream_t)stream) : sw_launch_c<K, 32>(p, (hipStream_t)stream);
}

extern "C" int gptst_stwa_lds_bytes(int N, int C) {
    if (N <= 0) return GPTST_EARG;
    if (C != 16 && C != 32) return GPTST_ESHAPE;
    size_t m = 0;
    for (int k = SW_K_LOCAL_FWD; k <= SW_K_LOCAL_BWD; ++k) m = std::max(m, sw_lds_any(k, N, C));      // the widest of the five launches
    return m > (size_t)1 << 30 ? GPTST_ESHAPE : (int)m;
}

extern "C" int gptst_stwa_slab_floats(int C) {
    if (C != 16 && C != 32) return GPTST_ESHAPE;
    return C == 16 ? SwSlab<16>::SIZE : SwSlab<32>::SIZE;
}

extern "C" int gptst_stwa_local_fwd(const float* h, const float* prox, const float* Y, const float* co, const float* cb, const float* V,
                                    const float* u, const float* WlT, const float* bl, float* Tq, float* Ks, float* Vs, int B, int T, int N, int C,
                                    int cuts, int cut, int cs, void* stream) {
    if (!h || !prox || !Y || !co || !cb || !V || !u || !WlT || !bl || !Tq || !Ks || !Vs) return GPTST_EARG;
    SwArgs p{};
    p.B = B; p.T = T; p.N = N; p.cuts = cuts; p.cut = cut; p.cs = cs;
    p.h = h; p.prox = prox; p.Y = const_cast<float*>(Y); p.co = co; p.cb = cb; p.V = V; p.u = u; p.WlT = WlT; p.bl = bl; p.Tq = Tq; p.Ks = Ks; p.Vs = Vs;
    return sw_launch<SW_K_LOCAL_FWD>(p, C, true, stream);
}

extern "C" int gptst_stwa_spatial_fwd(const float* Tq, const float* Ks, const float* Vs, const float* WlT, const float* bl, float* Y, float* S,
                                      float* mx, float* sm, int B, int N, int C, int cuts, int cut, void* stream) {
    if (!Tq || !Ks || !Vs || !WlT || !bl || !Y || (mx != nullptr) != (sm != nullptr)) return GPTST_EARG;
    SwArgs p{};
    p.B = B; p.N = N; p.cuts = cuts; p.cut = cut;
    p.Tq = const_cast<float*>(Tq); p.Ks = const_cast<float*>(Ks); p.Vs = const_cast<float*>(Vs); p.WlT = WlT; p.bl = bl; p.Y = Y; p.S = S; p.mx = mx; p.sm = sm;
    return sw_launch<SW_K_SPATIAL_FWD>(p, C, false, stream);
}

extern "C" int gptst_stwa_spatial_bwd_q(const float* Tq, const float* Ks, const float* Vs, const float* S, const float* mx, const float* sm,
                                        const float* Wl, const float* WlT, const float* bl, const float* dY, const float* carry, float* dS,
                                        float* Dq, float* dTq, float* slab, int B, int N, int C, int cuts, int cut, void* stream) {
    if (!Tq || !Ks || !Vs || !S || !mx || !sm || !Wl || !WlT || !bl || !dY || !dS || !Dq || !dTq) return GPTST_EARG;
    SwArgs p{};
    p.B = B; p.N = N; p.cuts = cuts; p.cut = cut;
    p.Tq = const_cast<float*>(Tq); p.Ks = const_cast<float*>(Ks); p.Vs = const_cast<float*>(Vs); p.S = const_cast<float*>(S);
    p.mx = const_cast<float*>(mx); p.sm = const_cast<float*>(sm); p.Wl = Wl; p.WlT = WlT; p.bl = bl; p.dY = dY; p.carry_in = carry;
    p.dS = dS; p.Dq = Dq; p.dTq = dTq; p.slab = slab;
    return sw_launch<SW_K_BWD_Q>(p, C, false, stream);
}

extern "C" int gptst_stwa_spatial_bwd_kv(const float* Tq, const float* Ks, const float* Vs, const float* dS, const float* Dq, const float* mx,
                                         const float* sm, float* dKs, float* dVs, int B, int N, int C, void* stream) {
    if (!Tq || !Ks || !Vs || !dS || !Dq || !mx || !sm || !dKs || !dVs) return GPTST_EARG;
    SwArgs p{};
    p.B = B; p.N = N; p.cuts = 1; p.cut = 0;
    p.Tq = const_cast<float*>(Tq); p.Ks = const_cast<float*>(Ks); p.Vs = const_cast<float*>(Vs); p.dS = const_cast<float*>(dS);
    p.Dq = const_cast<float*>(Dq); p.mx = const_cast<float*>(mx); p.sm = const_cast<float*>(sm); p.dKs = dKs; p.dVs = dVs;
    return sw_launch<SW_K_BWD_KV>(p, C, false, stream);
}

extern "C" int gptst_stwa_local_bwd(const float* h, const float* prox, const float* Y, const float* co, const float* cb, const float* V,
                                    const float* u, const float* Wl, const float* WlT, const float* bl, const float* dTq, const float* dKs,
                                    const float* dVs, float* dh, float* dPb, float* carry, float* dco, float* dcb, float* slab, int B, int T, int N,
                                    int C, int cuts, int cut, int cs, void* stream) {
    if (!h || !prox || !Y || !co || !cb || !V || !u || !Wl || !WlT || !bl || !dTq || !dKs || !dVs || !dco || !dcb) return GPTST_EARG;
    SwArgs p{};
    p.B = B; p.T = T; p.N = N; p.cuts = cuts; p.cut = cut; p.cs = cs;
    p.h = h; p.prox = prox; p.Y = const_cast<float*>(Y); p.co = co; p.cb = cb; p.V = V; p.u = u; p.Wl = Wl; p.WlT = WlT; p.bl = bl;
    p.dTq = const_cast<float*>(dTq); p.dKs = const_cast<float*>(dKs); p.dVs = const_cast<float*>(dVs);
    p.dh = dh; p.dPb = dPb; p.carry_out = carry; p.dco = dco; p.dcb = dcb; p.slab = slab;
    return sw_launch<SW_K_LOCAL_BWD>(p, C, true, stream);
}
