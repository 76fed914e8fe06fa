// The graph-GRU cell of the downstream CCRNN predictor (reference model/CCRNN_demand/CCRNN.py:39-60,198-233; gpt-st_amd/predictors/ccrnn.py) on
// HIP, forward and backward, at one graph-conv layer on one support.  With P_j = T_j(S) the Chebyshev polynomials of the learned graph as
// MATRICES (built once per forward, predictors/ccrnn_hip.py) a graph convolution of z is [z | P_1 z | .. | P_k z] W: the k products of a step
// are independent, one mix, not a chain.  The cell is TGCN's GRU step (csrc/tgcn.hip) with MSDR's multi-support mix (csrc/msdr.hip), on
// csrc/recur_step_dev.h as both are; one kernel family, two launches per cell step in each direction:
//
//   slab     In_b (all nodes of sample b), Ks <= 64 columns [state part (Hp) | input part (Cp)]
//   mix      M = [In | P_j[tile rows, :] In_b]_j             the identity block is the tile's own slab rows, as ms_step_kernel has it
//   GEMM     P = M Wt^T                                       Wt (NO, (k + 1) Ks) matrix-major, read from L2
//   epilogue TGCN's, in the accumulator layout, one of
//     fwd gates   In = [h | inp]     [r, u] = sigmoid(P + g);  writes u, q = r h, and (kept) r, M
//     fwd state   In = [q | inp]     c = tanh(P + g);          writes h' = u h + (1 - u) c, and (kept) c, M
//     bwd cand    In = dpre1 = (dh + dh2)(1 - u)(1 - c^2), formed on load and stored by the tile's owner;  P_j = P_j^T;  P = [dq | dinp];
//                                    writes dpre0 = [dq h r (1 - r) | dh (h - c) u (1 - u)], the partial dh = dh u + dq r, and dinp
//     bwd state   In = dpre0         P_j = P_j^T;  writes dh_{t-1} = partial + P[:, :Hp] and dinp += P[:, Hp:]
//   g is a hoisted seq tensor (the encoder: its input half runs over all B T units on the kernels of csrc/stgcn.hip, then Cp = 0) or a bias
//   vector (the decoder, whose input travels in the slab).
//
// The decoder's feedback: its input at step t is out(h_top of step t - 1), a (Cp, Hp) product far too small for a launch.  fwd gates forms it
// while the slab is filled — every workgroup for all nodes, in one fixed order, so all of them hold the same bits — and the tile's owner
// stores it (inp_out), where fwd state and the backward read it.
//
// Rows: a "step" tensor is (B*N, width) with row b N + n; a "seq" tensor is (B*T*N, width) with row (b T + t) N + n.  Hp = hidden_size
// zero-padded to a multiple of 16: a padded channel stays exactly 0 (sigmoid(0) = 1/2, tanh(0) = 0, h' = 0/2 + 0/2).  fp32 MFMA 16x16x4
// (exact fp32).  Plain launches only: no workgroup waits on another, no float atomics.
#include "common.h"
#include "gptst_hip.h"
#include "recur_step_dev.h"

#define CC_MAX_KS 3                  // polynomials T_1 .. T_k
#define CC_MAX_SLAB 64               // slab columns: one column group

enum { CC_FWD_GATES = 0, CC_FWD_STATE = 1, CC_BWD_CAND = 2, CC_BWD_STATE = 3 };

struct CcStep {
    const float* L; int Np, ks;                // (ks, Np, Np) zero-padded: P_j forward, P_j^T backward
    const float* Wt; int NO, K, Ks;            // (NO, K), K = (ks + 1) Ks: P = M Wt^T;  Ks slab columns
    int B, T, N, Hp, Cp, t;
    const float *h, *q, *u, *r, *c, *g, *bias, *dh, *dh2, *dp0, *inp, *dinp_in;
    const float *fb_h, *fb_W, *fb_b;           // fwd gates: inp = fb_h fb_W^T + fb_b formed on load (fb_h (B*N, Hp), fb_W (Cp, Hp), fb_b (Cp))
    float *u_out, *r_out, *q_out, *c_out, *h_out, *dp1_out, *dp0_out, *dh_out, *dinp_out, *inp_out;
    float* z;                                  // kept M -> z[seq row][col], pitch K (NULL: not kept)
};

// four columns of the fed-back input of node row `row`: fb_b + fb_W[o, :] . fb_h[row, :], summed in index order
__device__ __forceinline__ float4 cc_feedback(const CcStep& p, size_t row, int o) {
    float a[4] = {p.fb_b[o], p.fb_b[o + 1], p.fb_b[o + 2], p.fb_b[o + 3]};
    const float* hp = p.fb_h + row * p.Hp;
    for (int i = 0; i < p.Hp; i += 4) {
        const float4 hv = ld4(hp + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float4 w = ld4(p.fb_W + (size_t)(o + e) * p.Hp + i);
            a[e] += hv.x * w.x;
            a[e] += hv.y * w.y;
            a[e] += hv.z * w.z;
            a[e] += hv.w * w.w;
        }
    }
    return make_float4(a[0], a[1], a[2], a[3]);
}

template <int MODE, int NT>
__global__ __launch_bounds__(RECUR_THREADS) void cc_step_kernel(CcStep p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* slab = smem;                              // [Np][RECUR_SP]: In_b
    const int MP = p.K + 4;
    float* Ml = smem + (size_t)p.Np * RECUR_SP;      // [16 NT][K + 4]: M, the A operand of the GEMM
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int b = blockIdx.y, n0 = blockIdx.x * 16 * NT, Hp = p.Hp, Cp = p.Cp, Ks = p.Ks;
    const size_t srow = (size_t)b * p.N;                         // first step row of b
    const size_t qrow = ((size_t)b * p.T + p.t) * p.N;           // first seq row of (b, t)
    bool tv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) tv[nt] = n0 + 16 * nt < p.Np;

    // ---- the slab: Ks <= 64 columns of In_b ----
    for (int f = tid; f < p.Np * 16; f += RECUR_THREADS) {
        const int m = f >> 4, c4 = f & 15, col = 4 * c4;
        float4 v = f4zero();
        if (m < p.N && col < Ks) {
            if (MODE <= CC_FWD_STATE) {
                if (col < Hp) {
                    v = ld4((MODE == CC_FWD_GATES ? p.h : p.q) + (srow + m) * Hp + col);
                } else if (MODE == CC_FWD_GATES && p.fb_h != nullptr) {
                    v = cc_feedback(p, srow + m, col - Hp);
                    if (m >= n0 && m < n0 + 16 * NT) st4(p.inp_out + (srow + m) * Cp + col - Hp, v);     // the tile's owner keeps the input
                } else {
                    v = ld4(p.inp + (srow + m) * Cp + col - Hp);
                }
            } else if (MODE == CC_BWD_STATE) {
                v = ld4(p.dp0 + (qrow + m) * 2 * Hp + col);
            } else {
                float4 d = ld4(p.dh + (srow + m) * Hp + col);
                if (p.dh2 != nullptr) {
                    const float4 e = ld4(p.dh2 + (srow + m) * Hp + col);
                    d = make_float4(d.x + e.x, d.y + e.y, d.z + e.z, d.w + e.w);
                }
                const float4 u = ld4(p.u + (srow + m) * Hp + col), c = ld4(p.c + (srow + m) * Hp + col);
                v = make_float4(d.x * (1.f - u.x) * (1.f - c.x * c.x), d.y * (1.f - u.y) * (1.f - c.y * c.y),
                                d.z * (1.f - u.z) * (1.f - c.z * c.z), d.w * (1.f - u.w) * (1.f - c.w * c.w));
                if (m >= n0 && m < n0 + 16 * NT) st4(p.dp1_out + (qrow + m) * Hp + col, v);              // the tile's owner keeps dpre1
            }
        }
        st4(slab + m * RECUR_SP + col, v);
    }
    __syncthreads();

    // ---- mix: M = [In | P_j[tile rows, :] In_b]_j; wave w owns column tile w of the slab for all NT row tiles ----
    for (int f = tid; f < 16 * NT * 16; f += RECUR_THREADS) {    // the identity block: the tile's own rows
        const int row = f >> 4, c4 = f & 15, col = 4 * c4, n = n0 + row;
        if (col >= Ks) continue;
        const float4 v = n < p.Np ? ld4(slab + n * RECUR_SP + col) : f4zero();
        st4(Ml + row * MP + col, v);
        if (MODE <= CC_FWD_STATE && p.z != nullptr && n < p.N) st4(p.z + (qrow + n) * p.K + col, v);
    }
    if (16 * wave < Ks) {                                        // (wave-uniform)
        for (int k = 0; k < p.ks; ++k) {
            f32x4 acc[NT];
            recur_mix_tiles<NT>(acc, p.L + (size_t)k * p.Np * p.Np, p.Np, n0, tv, slab, wave, j, kk);
            const int col = (k + 1) * Ks + 16 * wave + j;        // accumulator layout: reg r = (row 4 kk + r, column j)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * nt + 4 * kk + r, n = n0 + row;
                    Ml[row * MP + col] = acc[nt][r];
                    if (MODE <= CC_FWD_STATE && p.z != nullptr && n < p.N) p.z[(qrow + n) * p.K + col] = acc[nt][r];
                }
        }
    }
    __syncthreads();

    // ---- GEMM + epilogue: wave w owns output column tiles w, w + 4, ... for all NT row tiles ----
    for (int ct = wave; 16 * ct < p.NO; ct += RECUR_THREADS / 64) {
        f32x4 acc[NT];
        recur_gemm_tiles<NT>(acc, Ml, MP, p.Wt, p.K, ct, j, kk);
        const int col = 16 * ct + j;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + 16 * nt + 4 * kk + r;
                if (n >= p.N) continue;
                const float v = acc[nt][r];
                if (MODE == CC_FWD_GATES) {
                    const float s = sigmoidf_(v + (p.g != nullptr ? p.g[(qrow + n) * 2 * Hp + col] : p.bias[col]));
                    if (col < Hp) {                                                  // reset gate
                        const size_t i = (srow + n) * Hp + col;
                        if (p.r_out != nullptr) p.r_out[i] = s;
                        p.q_out[i] = s * p.h[i];
                    } else {
                        p.u_out[(srow + n) * Hp + col - Hp] = s;                     // update gate
                    }
                } else if (MODE == CC_FWD_STATE) {
                    const size_t i = (srow + n) * Hp + col;
                    const float c = tanhf(v + (p.g != nullptr ? p.g[(qrow + n) * Hp + col] : p.bias[col])), u = p.u[i];
                    if (p.c_out != nullptr) p.c_out[i] = c;
                    p.h_out[i] = u * p.h[i] + (1.f - u) * c;
                } else if (col >= Hp) {                                              // the gradient of the cell's input
                    const size_t i = (srow + n) * Cp + col - Hp;
                    p.dinp_out[i] = MODE == CC_BWD_CAND ? v : p.dinp_in[i] + v;
                } else if (MODE == CC_BWD_CAND) {
                    const size_t i = (srow + n) * Hp + col;
                    const float h = p.h[i], rr = p.r[i], u = p.u[i], c = p.c[i], d = p.dh[i] + (p.dh2 != nullptr ? p.dh2[i] : 0.f);
                    float* o = p.dp0_out + (qrow + n) * 2 * Hp + col;
                    o[0] = v * h * (rr * (1.f - rr));
                    o[Hp] = d * (h - c) * (u * (1.f - u));
                    p.dh_out[i] = d * u + v * rr;
                } else {
                    const size_t i = (srow + n) * Hp + col;
                    p.dh_out[i] = p.dh[i] + v;
                }
            }
    }
}

// ---- launch ----
static size_t cc_lds_bytes(int Np, int K, int nt) { return ((size_t)Np * RECUR_SP + (size_t)16 * nt * (K + 4)) * sizeof(float); }

static int cc_shape(int Hp, int Cp, int ks) {
    if (ks < 1 || ks > CC_MAX_KS || Hp < 16 || Hp > 32 || Hp % 16 || Cp < 0 || Cp % 16 || Hp + Cp > CC_MAX_SLAB) return GPTST_ESHAPE;
    return GPTST_OK;
}

template <int MODE>
static int cc_launch(CcStep p, int tiles, void* stream) {
    if (!p.L) return GPTST_EARG;
    int rc = recur_check(p.Wt, p.B, p.T, p.N, p.t, tiles, p.Hp, p.Np);
    if (rc == GPTST_OK) rc = cc_shape(p.Hp, p.Cp, p.ks);
    if (rc != GPTST_OK) return rc;
    p.K = (p.ks + 1) * p.Ks;
    const int nt = recur_tiles(p.B, p.Np, tiles);
    const size_t smem = cc_lds_bytes(p.Np, p.K, nt);
    if (smem > RECUR_LDS_MAX) return GPTST_ESHAPE;
    const dim3 grid((p.Np / 16 + nt - 1) / nt, p.B);
    return nt == 2 ? recur_launch<cc_step_kernel<MODE, 2>>(p, grid, smem, (hipStream_t)stream)
                   : recur_launch<cc_step_kernel<MODE, 1>>(p, grid, smem, (hipStream_t)stream);
}

extern "C" int gptst_ccrnn_lds_bytes(int N, int Hp, int Cp, int ks, int B) {
    if (N <= 0 || Hp <= 0 || Cp < 0 || ks <= 0 || B <= 0) return GPTST_EARG;
    if (cc_shape(Hp, Cp, ks) != GPTST_OK) return GPTST_ESHAPE;
    const int Np = 16 * ((N + 15) / 16), wide = Hp + Cp > 2 * Hp ? Hp + Cp : 2 * Hp;      // the widest slab of the four launches
    return (int)cc_lds_bytes(Np, (ks + 1) * wide, recur_tiles(B, Np, 0));
}

extern "C" int gptst_ccrnn_fwd_gates(const float* P, int Np, int ks, const float* W0, const float* h, const float* inp, int Cp, const float* fb_h,
                                     const float* fb_W, const float* fb_b, float* inp_out, const float* Gx0, const float* bias, float* u, float* r,
                                     float* q, float* z, int B, int T, int N, int Hp, int t, int tiles, void* stream) {
    if (!h || !u || !q || q == h || u == h || r == h || (Gx0 == nullptr) == (bias == nullptr)) return GPTST_EARG;
    if (Cp > 0 && ((fb_h == nullptr) == (inp == nullptr) || (fb_h != nullptr && (!fb_W || !fb_b || !inp_out || inp_out == fb_h)))) return GPTST_EARG;
    if (Cp <= 0 && (fb_h != nullptr || inp != nullptr)) return GPTST_EARG;
    CcStep p{};
    p.L = P; p.Np = Np; p.ks = ks; p.Wt = W0; p.NO = 2 * Hp; p.Ks = Hp + Cp; p.B = B; p.T = T; p.N = N; p.Hp = Hp; p.Cp = Cp; p.t = t;
    p.h = h; p.inp = inp; p.fb_h = fb_h; p.fb_W = fb_W; p.fb_b = fb_b; p.inp_out = inp_out; p.g = Gx0; p.bias = bias;
    p.u_out = u; p.r_out = r; p.q_out = q; p.z = z;
    return cc_launch<CC_FWD_GATES>(p, tiles, stream);
}

extern "C" int gptst_ccrnn_fwd_state(const float* P, int Np, int ks, const float* W1, const float* q, const float* inp, int Cp, const float* Gx1,
                                     const float* bias, const float* u, const float* h, float* h_out, float* c, float* z, int B, int T, int N,
                                     int Hp, int t, int tiles, void* stream) {
    if (!q || !u || !h || !h_out || h_out == q || h_out == h || (Gx1 == nullptr) == (bias == nullptr) || (Cp > 0) != (inp != nullptr)) return GPTST_EARG;
    CcStep p{};
    p.L = P; p.Np = Np; p.ks = ks; p.Wt = W1; p.NO = Hp; p.Ks = Hp + Cp; p.B = B; p.T = T; p.N = N; p.Hp = Hp; p.Cp = Cp; p.t = t;
    p.q = q; p.inp = inp; p.g = Gx1; p.bias = bias; p.u = u; p.h = h; p.h_out = h_out; p.c_out = c; p.z = z;
    return cc_launch<CC_FWD_STATE>(p, tiles, stream);
}

extern "C" int gptst_ccrnn_bwd_cand(const float* PT, int Np, int ks, const float* W1T, int Cp, const float* dh, const float* dh2, const float* u,
                                    const float* c, const float* r, const float* h, float* dpre1, float* dpre0, float* dh_part, float* dinp, int B,
                                    int T, int N, int Hp, int t, int tiles, void* stream) {
    if (!dh || !u || !c || !r || !h || !dpre1 || !dpre0 || !dh_part || dh_part == dh || dh_part == dh2 || (Cp > 0) != (dinp != nullptr)) return GPTST_EARG;
    CcStep p{};
    p.L = PT; p.Np = Np; p.ks = ks; p.Wt = W1T; p.NO = Hp + Cp; p.Ks = Hp; p.B = B; p.T = T; p.N = N; p.Hp = Hp; p.Cp = Cp; p.t = t;
    p.dh = dh; p.dh2 = dh2; p.u = u; p.c = c; p.r = r; p.h = h; p.dp1_out = dpre1; p.dp0_out = dpre0; p.dh_out = dh_part; p.dinp_out = dinp;
    return cc_launch<CC_BWD_CAND>(p, tiles, stream);
}

extern "C" int gptst_ccrnn_bwd_state(const float* PT, int Np, int ks, const float* W0T, int Cp, const float* dpre0, const float* dh_part,
                                     float* dh_out, float* dinp, int B, int T, int N, int Hp, int t, int tiles, void* stream) {
    if (!dpre0 || !dh_part || !dh_out || dh_out == dh_part || (Cp > 0) != (dinp != nullptr)) return GPTST_EARG;
    CcStep p{};
    p.L = PT; p.Np = Np; p.ks = ks; p.Wt = W0T; p.NO = Hp + Cp; p.Ks = 2 * Hp; p.B = B; p.T = T; p.N = N; p.Hp = Hp; p.Cp = Cp; p.t = t;
    p.dp0 = dpre0; p.dh = dh_part; p.dh_out = dh_out; p.dinp_in = dinp; p.dinp_out = dinp;
    return cc_launch<CC_BWD_STATE>(p, tiles, stream);
}
