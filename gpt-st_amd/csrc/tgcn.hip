// The recurrence of the downstream TGCN predictor (reference model/TGCN/TGCN.py:70-91; gpt-st_amd/predictors/tgcn.py) on HIP, forward and
// backward.  Everything outside the h chain is hoisted out of the loop onto the STGCN kernels (csrc/stgcn.hip: nodemix, tapgemm, wgrad); what is
// left per step is one kernel family, two launches per step in each direction:
//
//   mix      M = L[tile rows, :] In_b          the workgroup's 16-node tiles against ALL nodes of its batch element b (hence a launch boundary
//                                              after every use: the next mix needs every tile's output)
//   GEMM     P = M Wt^T                        Wt (NO, K) row-major, read from L2 (every row tile needs all of it once)
//   epilogue in the accumulator layout, one of
//     fwd gates   In = h          [r, u] = sigmoid(P + Gx0_t);  writes u, q = r h, and (kept) r, m1 = M
//     fwd state   In = q          c = tanh(P + Gx1_t);          writes h' = u h + (1 - u) c, and (kept) c, m2 = M
//     bwd cand    In = dpre1 = dh' (1 - u)(1 - c^2), formed on load and stored by the tile's owner;  L = L^T, P = dq;
//                                 writes dpre0 = [dq h r (1 - r) | dh' (h - c) u (1 - u)] and the partial dh = dh' u + dq r
//     bwd state   In = dpre0      L = L^T;  writes dh_{t-1} = partial + P
//
// Rows: a "step" tensor is (B*N, Hp) with row b N + n; a "seq" tensor is (B*T*N, width) with row (b T + t) N + n (the layout of the hoisted
// kernels: channels-last, nothing permuted).  Hp = rnn_units zero-padded to a multiple of 16: a padded channel stays exactly 0 (sigmoid(0) = 1/2,
// tanh(0) = 0, h' = 0/2 + 0/2).  fp32 MFMA 16x16x4 (exact fp32).  Plain launches only: no workgroup waits on another, no float atomics.
// The GEMM's inner loop, the constants and the launch are csrc/recur_step_dev.h's, shared with csrc/msdr.hip; the slab fill, the mix loop (the
// header's recur_mix_tiles, kept written out here: measured) and the epilogues are here.
#include "common.h"
#include "gptst_hip.h"
#include "recur_step_dev.h"

enum { TG_FWD_GATES = 0, TG_FWD_STATE = 1, TG_BWD_CAND = 2, TG_BWD_STATE = 3 };

struct TgStep {
    const float* L; int Np;                    // (Np, Np) zero-padded: L forward, L^T backward
    const float* Wt; int NO, K;                // (NO, K): P = M Wt^T
    int B, T, N, Hp, t;
    const float *h, *q, *u, *r, *c, *g, *dh, *dp0;          // inputs by role (see the table above); g = Gx0 / Gx1 (seq)
    float *u_out, *r_out, *q_out, *c_out, *h_out, *dp1_out, *dp0_out, *dh_out;
    float* z; int ldz, zoff;                   // kept M -> z[seq row][zoff + col] (NULL: not kept)
};

template <int MODE, int NT>
__global__ __launch_bounds__(RECUR_THREADS) void tg_step_kernel(TgStep p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* slab = smem;                              // [Np][RECUR_SP]: 64 columns of In_b
    const int MP = p.K + 4;
    float* Ml = smem + (size_t)p.Np * RECUR_SP;      // [16 NT][K + 4]: M, the A operand of the GEMM
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int b = blockIdx.y, n0 = blockIdx.x * 16 * NT, Hp = p.Hp;
    const size_t srow = (size_t)b * p.N;                         // first step row of b
    const size_t qrow = ((size_t)b * p.T + p.t) * p.N;           // first seq row of (b, t)
    bool tv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) tv[nt] = n0 + 16 * nt < p.Np;

    // ---- mix: M = L[tile rows, :] In_b, 64 columns of In_b at a time; wave w owns column tile w of the 64 for all NT row tiles ----
    for (int cg = 0; 64 * cg < p.K; ++cg) {
        __syncthreads();                                         // the previous slab's reads are done
        for (int f = tid; f < p.Np * 16; f += RECUR_THREADS) {
            const int m = f >> 4, c4 = f & 15, col = 64 * cg + 4 * c4;
            float4 v = f4zero();
            if (m < p.N && col < p.K) {
                if (MODE == TG_FWD_GATES) v = ld4(p.h + (srow + m) * Hp + col);
                else if (MODE == TG_FWD_STATE) v = ld4(p.q + (srow + m) * Hp + col);
                else if (MODE == TG_BWD_STATE) v = ld4(p.dp0 + (qrow + m) * 2 * Hp + col);
                else {
                    const float4 d = ld4(p.dh + (srow + m) * Hp + col), u = ld4(p.u + (srow + m) * Hp + col), c = ld4(p.c + (srow + m) * Hp + col);
                    v = make_float4(d.x * (1.f - u.x) * (1.f - c.x * c.x), d.y * (1.f - u.y) * (1.f - c.y * c.y),
                                    d.z * (1.f - u.z) * (1.f - c.z * c.z), d.w * (1.f - u.w) * (1.f - c.w * c.w));
                    if (m >= n0 && m < n0 + 16 * NT) st4(p.dp1_out + (qrow + m) * Hp + col, v);      // the tile's owner keeps dpre1
                }
            }
            st4(slab + m * RECUR_SP + 4 * c4, v);
        }
        __syncthreads();
        if (64 * cg + 16 * wave >= p.K) continue;                // (wave-uniform)
        // recur_mix_tiles, written out: through the shared function these kernels came out 0.5 - 1.3 % slower (recur_step_dev.h)
        f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        float4 an[NT];                                             // the graph rows come from L2: fetched one step ahead of their use
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) an[nt] = tv[nt] ? ld4(p.L + (size_t)(n0 + 16 * nt + j) * p.Np + 4 * kk) : f4zero();
        for (int m0 = 0; m0 < p.Np; m0 += 16) {
            float4 a[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                a[nt] = an[nt];
                if (tv[nt] && m0 + 16 < p.Np) an[nt] = ld4(p.L + (size_t)(n0 + 16 * nt + j) * p.Np + m0 + 16 + 4 * kk);
            }
            const float* sp = slab + (m0 + 4 * kk) * RECUR_SP + 16 * wave + j;
            const float bv[4] = {sp[0], sp[RECUR_SP], sp[2 * RECUR_SP], sp[3 * RECUR_SP]};
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt].x, bv[0], acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt].y, bv[1], acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt].z, bv[2], acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[nt].w, bv[3], acc[nt], 0, 0, 0);
            }
        }
        const int col = 64 * cg + 16 * wave + j;                 // accumulator layout: reg r = (row 4 kk + r, column j)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * nt + 4 * kk + r, n = n0 + row;
                Ml[row * MP + col] = acc[nt][r];
                if (MODE <= TG_FWD_STATE && p.z != nullptr && n < p.N) p.z[(qrow + n) * p.ldz + p.zoff + col] = acc[nt][r];
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
                if (MODE == TG_FWD_GATES) {
                    const float s = sigmoidf_(v + p.g[(qrow + n) * 2 * Hp + col]);
                    if (col < Hp) {                                                  // reset gate
                        const size_t i = (srow + n) * Hp + col;
                        if (p.r_out != nullptr) p.r_out[i] = s;
                        p.q_out[i] = s * p.h[i];
                    } else {
                        p.u_out[(srow + n) * Hp + col - Hp] = s;                     // update gate
                    }
                } else if (MODE == TG_FWD_STATE) {
                    const size_t i = (srow + n) * Hp + col;
                    const float c = tanhf(v + p.g[(qrow + n) * Hp + col]), u = p.u[i];
                    if (p.c_out != nullptr) p.c_out[i] = c;
                    p.h_out[i] = u * p.h[i] + (1.f - u) * c;
                } else if (MODE == TG_BWD_CAND) {
                    const size_t i = (srow + n) * Hp + col;
                    const float h = p.h[i], rr = p.r[i], u = p.u[i], c = p.c[i], d = p.dh[i];
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
static size_t tg_lds_bytes(int Np, int K, int nt) { return ((size_t)Np * RECUR_SP + (size_t)16 * nt * (K + 4)) * sizeof(float); }

template <int MODE>
static int tg_launch(TgStep p, int tiles, void* stream) {
    if (!p.L) return GPTST_EARG;
    const int rc = recur_check(p.Wt, p.B, p.T, p.N, p.t, tiles, p.Hp, p.Np);
    if (rc != GPTST_OK) return rc;
    const int nt = recur_tiles(p.B, p.Np, tiles);
    const size_t smem = tg_lds_bytes(p.Np, p.K, nt);
    if (smem > RECUR_LDS_MAX) return GPTST_ESHAPE;
    const dim3 grid((p.Np / 16 + nt - 1) / nt, p.B);
    return nt == 2 ? recur_launch<tg_step_kernel<MODE, 2>>(p, grid, smem, (hipStream_t)stream)
                   : recur_launch<tg_step_kernel<MODE, 1>>(p, grid, smem, (hipStream_t)stream);
}

extern "C" int gptst_tgcn_lds_bytes(int N, int Hp, int B) {
    if (N <= 0 || Hp <= 0 || B <= 0) return GPTST_EARG;
    const int Np = 16 * ((N + 15) / 16);
    return (int)tg_lds_bytes(Np, 2 * Hp, recur_tiles(B, Np, 0));               // the widest K of the four launches (bwd state)
}

extern "C" int gptst_tgcn_fwd_gates(const float* L, int Np, const float* W0h, const float* h, const float* Gx0, float* u, float* r, float* q,
                                    float* z, int ldz, int zoff, int B, int T, int N, int Hp, int t, int tiles, void* stream) {
    if (!h || !Gx0 || !u || !q || q == h || u == h || r == h || (z != nullptr && (zoff < 0 || ldz < zoff + Hp || ldz % 4 || zoff % 4))) return GPTST_EARG;
    TgStep p{};
    p.L = L; p.Np = Np; p.Wt = W0h; p.NO = 2 * Hp; p.K = Hp; p.B = B; p.T = T; p.N = N; p.Hp = Hp; p.t = t;
    p.h = h; p.g = Gx0; p.u_out = u; p.r_out = r; p.q_out = q; p.z = z; p.ldz = ldz; p.zoff = zoff;
    return tg_launch<TG_FWD_GATES>(p, tiles, stream);
}

extern "C" int gptst_tgcn_fwd_state(const float* L, int Np, const float* W1h, const float* q, const float* Gx1, const float* u, const float* h,
                                    float* h_out, float* c, float* z, int ldz, int zoff, int B, int T, int N, int Hp, int t, int tiles,
                                    void* stream) {
    if (!q || !Gx1 || !u || !h || !h_out || h_out == q || (z != nullptr && (zoff < 0 || ldz < zoff + Hp || ldz % 4 || zoff % 4))) return GPTST_EARG;
    TgStep p{};
    p.L = L; p.Np = Np; p.Wt = W1h; p.NO = Hp; p.K = Hp; p.B = B; p.T = T; p.N = N; p.Hp = Hp; p.t = t;
    p.q = q; p.g = Gx1; p.u = u; p.h = h; p.h_out = h_out; p.c_out = c; p.z = z; p.ldz = ldz; p.zoff = zoff;
    return tg_launch<TG_FWD_STATE>(p, tiles, stream);
}

extern "C" int gptst_tgcn_bwd_cand(const float* LT, int Np, const float* W1hT, const float* dh, const float* u, const float* c, const float* r,
                                   const float* h, float* dpre1, float* dpre0, float* dh_part, int B, int T, int N, int Hp, int t, int tiles,
                                   void* stream) {
    if (!dh || !u || !c || !r || !h || !dpre1 || !dpre0 || !dh_part || dh_part == dh) return GPTST_EARG;
    TgStep p{};
    p.L = LT; p.Np = Np; p.Wt = W1hT; p.NO = Hp; p.K = Hp; p.B = B; p.T = T; p.N = N; p.Hp = Hp; p.t = t;
    p.dh = dh; p.u = u; p.c = c; p.r = r; p.h = h; p.dp1_out = dpre1; p.dp0_out = dpre0; p.dh_out = dh_part;
    return tg_launch<TG_BWD_CAND>(p, tiles, stream);
}

extern "C" int gptst_tgcn_bwd_state(const float* LT, int Np, const float* W0hT, const float* dpre0, const float* dh_part, float* dh_out, int B,
                                    int T, int N, int Hp, int t, int tiles, void* stream) {
    if (!dpre0 || !dh_part || !dh_out) return GPTST_EARG;
    TgStep p{};
    p.L = LT; p.Np = Np; p.Wt = W0hT; p.NO = Hp; p.K = 2 * Hp; p.B = B; p.T = T; p.N = N; p.Hp = Hp; p.t = t;
    p.dp0 = dpre0; p.dh = dh_part; p.dh_out = dh_out;
    return tg_launch<TG_BWD_STATE>(p, tiles, stream);
}
