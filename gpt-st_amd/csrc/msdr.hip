// The multi-state recurrence of the downstream MSDR predictor (reference model/MSDR/gmsdr_cell.py:109-186; gpt-st_amd/predictors/msdr.py) on HIP,
// forward and backward.  A cell keeps its last K outputs; with h = the newest of them one application is
//
//     pre = Gx_t + [h, L_1 h, .., A h] Th          c = leaky_relu(pre)          e_k = w . vec(s_k + R_k) + bias,  a = softmax_k(e)
//     o   = c W + b + sum_k a_k (s_k + R_k)
//
// Everything on the input side (Gx = [U, L U, A U] Tx + beta over all steps, every weight / graph / input gradient) is hoisted out of the loop
// onto the kernels of csrc/stgcn.hip and csrc/mtgnn.hip (predictors/msdr_hip.py).  What is left per step is this kernel family, in the layout of
// csrc/recur_step_dev.h (whose two inner loops and launch it shares with csrc/tgcn.hip): a workgroup owns 16 NT nodes of one sample b;
//
//   fwd step    1 launch   slab = h_b (all nodes) in LDS;  M = [h | L_k h]_k for the tile;  pre = M Wh^T + Gx_t;  c -> LDS;  o = c W2^T + b +
//                          the attention mix;  writes o into the state ring's next slot and, per workgroup, sigma = w . o over its tile
//                          (and the same against a second vector w2: the decoder cell that will start from these states has its own w).
//                          The logits of the K states come from those partials: folded in index order by every workgroup of b in the
//                          prologue of the launch that reads them (no float atomics: a repeated run is bit-identical).
//   bwd pre     launch 1   dc = dO W^T, dpre = dc leaky'(c);  per workgroup and k the partial <dO, s_k + R_k> over its tile
//   bwd state   launch 2   folds the partials: dA_k, de = a (dA - sum a dA);  slab = dpre_b;  dh = [dpre | L_k^T dpre]_k Wh'^T;
//                          dS_k += a_k dO + de_k w  (k = K - 1: + dh) — the gradient ring, every element owned by one thread
//   (two launches: de needs every tile's partial, dh needs every tile's dpre.)
//
// Rows: everything is time-major, row (t B + b) N + n of a (T B N, width) tensor; the state ring Hs is (T + K, B N, Hp): slots [0, K) the
// initial states, oldest first, slot K + t the output of step t, so step t reads slots t .. t + K - 1 and Hs[K:] is the output sequence.
// Hp = rnn_units zero-padded to a multiple of 16: a padded channel stays exactly 0 (its Gx, Wh, W2, b, R are 0: leaky_relu(0) W + 0 + sum a 0).
// fp32 MFMA 16x16x4 (exact fp32).  Plain launches only: no workgroup waits on another.
#include "common.h"
#include "gptst_hip.h"
#include "recur_step_dev.h"

#define MS_MAXK 8                // kept states

enum { MS_FWD = 0, MS_BWD_PRE = 1, MS_BWD_STATE = 2 };

struct MsStep {
    const float* L; int Np, ks;                // (ks, Np, Np) zero-padded: the fixed supports then A (forward), their transposes (backward)
    const float* Wt; int NO, K;                // (NO, K): P = M Wt^T
    const float* W2;                           // fwd: (Hp, Hp) = W^T
    int B, T, N, Hp, t, Kk, G;                 // Kk kept states; G = workgroups per sample (the length of a partial row)
    const float *g, *bvec, *R, *w, *w2, *wr;   // Gx (seq); b (N, Hp); R (Kk, N, Hp); attention weights (N, Hp); wr (Kk) = w . R_k + bias
    float* Hs;                                 // fwd: the state ring (read slots t .. t + Kk - 1, write slot t + Kk);  bwd pre: read only
    float *sig, *sig2;                         // (T + Kk, B, G) partials of w . s and w2 . s (sig2 may be NULL)
    float *c, *z, *a;                          // fwd: kept c (seq), M (seq, ldz), a (T, B, Kk) — each may be NULL;  bwd: c, a read
    int ldz;
    float* dH;                                 // the gradient ring (T + Kk, B N, Hp)
    float *dpre, *pa, *de;                     // dpre (seq);  pa (B, G, MS_MAXK);  de (T, B, Kk)
};

// fixed-order sum over the workgroup (every thread calls it): lanes by xor-shuffle, the four waves in index order
__device__ __forceinline__ float ms_block_sum(float v, float* red, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

template <int MODE, int NT>
__global__ __launch_bounds__(RECUR_THREADS) void ms_step_kernel(MsStep p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float att[MS_MAXK], dev[MS_MAXK], red[4];
    const int MP = p.K + 4, CP = p.Hp + 4;
    float* slab = smem;                                                     // [Np][RECUR_SP]: 64 columns of In_b (not in bwd pre)
    float* Ml = smem + (MODE == MS_BWD_PRE ? 0 : (size_t)p.Np * RECUR_SP);  // [16 NT][K + 4]: the A operand of the GEMM
    float* Cl = Ml + (size_t)16 * NT * MP;                                  // fwd: [16 NT][Hp + 4]: c, the A operand of the second GEMM
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int b = blockIdx.y, n0 = blockIdx.x * 16 * NT, Hp = p.Hp, Kk = p.Kk;
    const size_t slot = (size_t)p.B * p.N * Hp;                          // floats per ring slot
    const size_t srow = (size_t)b * p.N;                                 // first row of b inside a slot
    const size_t qrow = ((size_t)p.t * p.B + b) * p.N;                   // first seq row of (t, b)
    bool tv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) tv[nt] = n0 + 16 * nt < p.Np;

    // ---- prologue: the attention weights of this sample (fwd), or de from the partials of launch 1 (bwd state) ----
    if (MODE == MS_FWD) {
        if (tid < Kk) {
            const float* sp = p.sig + ((size_t)(p.t + tid) * p.B + b) * p.G;
            float e = 0.f;
            for (int gi = 0; gi < p.G; ++gi) e += sp[gi];
            dev[tid] = e + p.wr[tid];
        }
        __syncthreads();
        if (tid == 0) {
            float mx = dev[0], s = 0.f;
            for (int k = 1; k < Kk; ++k) mx = fmaxf(mx, dev[k]);
            for (int k = 0; k < Kk; ++k) { att[k] = expf(dev[k] - mx); s += att[k]; }
            for (int k = 0; k < Kk; ++k) {
                att[k] /= s;
                if (p.a != nullptr && blockIdx.x == 0) p.a[((size_t)p.t * p.B + b) * Kk + k] = att[k];
            }
        }
    } else if (MODE == MS_BWD_STATE) {
        if (tid < Kk) {
            const float* pp = p.pa + (size_t)b * p.G * MS_MAXK + tid;
            float s = 0.f;
            for (int gi = 0; gi < p.G; ++gi) s += pp[(size_t)gi * MS_MAXK];
            dev[tid] = s;                                                 // dA_k
            att[tid] = p.a[((size_t)p.t * p.B + b) * Kk + tid];
        }
        __syncthreads();
        if (tid == 0) {
            float dot = 0.f;
            for (int k = 0; k < Kk; ++k) dot += att[k] * dev[k];
            for (int k = 0; k < Kk; ++k) {
                dev[k] = att[k] * (dev[k] - dot);                         // de_k
                if (blockIdx.x == 0) p.de[((size_t)p.t * p.B + b) * Kk + k] = dev[k];
            }
        }
    }

    if (MODE == MS_BWD_PRE) {
        // ---- the A operand is the tile's own rows of dO = dH[slot Kk + t] ----
        const float* dO = p.dH + (size_t)(Kk + p.t) * slot;
        for (int f = tid; f < 16 * NT * (Hp / 4); f += RECUR_THREADS) {
            const int row = f / (Hp / 4), c4 = f % (Hp / 4), n = n0 + row;
            st4(Ml + row * MP + 4 * c4, n < p.N ? ld4(dO + (srow + n) * Hp + 4 * c4) : f4zero());
        }
    } else {
        // ---- mix: M = [In | L_k[tile rows, :] In_b]_k, 64 columns of In_b at a time; wave w owns column tile w of the 64 for all NT row tiles ----
        const float* In = MODE == MS_FWD ? p.Hs + (size_t)(p.t + Kk - 1) * slot + srow * Hp : p.dpre + qrow * Hp;
        for (int cg = 0; 64 * cg < Hp; ++cg) {
            __syncthreads();                                             // the previous slab's reads are done (and the prologue's writes)
            for (int f = tid; f < p.Np * 16; f += RECUR_THREADS) {
                const int m = f >> 4, c4 = f & 15, col = 64 * cg + 4 * c4;
                st4(slab + m * RECUR_SP + 4 * c4, (m < p.N && col < Hp) ? ld4(In + (size_t)m * Hp + col) : f4zero());
            }
            __syncthreads();
            for (int f = tid; f < 16 * NT * 16; f += RECUR_THREADS) {    // the identity block: the tile's own rows
                const int row = f >> 4, c4 = f & 15, col = 64 * cg + 4 * c4, n = n0 + row;
                if (col >= Hp) continue;
                const float4 v = n < p.Np ? ld4(slab + n * RECUR_SP + 4 * c4) : f4zero();
                st4(Ml + row * MP + col, v);
                if (MODE == MS_FWD && p.z != nullptr && n < p.N) st4(p.z + (qrow + n) * p.ldz + col, v);
            }
            if (64 * cg + 16 * wave >= Hp) continue;                     // (wave-uniform)
            for (int k = 0; k < p.ks; ++k) {
                f32x4 acc[NT];
                recur_mix_tiles<NT>(acc, p.L + (size_t)k * p.Np * p.Np, p.Np, n0, tv, slab, wave, j, kk);
                const int col = (k + 1) * Hp + 64 * cg + 16 * wave + j;  // accumulator layout: reg r = (row 4 kk + r, column j)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * nt + 4 * kk + r, n = n0 + row;
                        Ml[row * MP + col] = acc[nt][r];
                        if (MODE == MS_FWD && p.z != nullptr && n < p.N) p.z[(qrow + n) * p.ldz + col] = acc[nt][r];
                    }
            }
        }
    }
    __syncthreads();

    // ---- GEMM + epilogue: wave w owns output column tiles w, w + 4, ... for all NT row tiles ----
    float part[MS_MAXK];
#pragma unroll
    for (int k = 0; k < MS_MAXK; ++k) part[k] = 0.f;
    for (int ct = wave; 16 * ct < p.NO; ct += RECUR_THREADS / 64) {
        f32x4 acc[NT];
        recur_gemm_tiles<NT>(acc, Ml, MP, p.Wt, p.K, ct, j, kk);
        const int col = 16 * ct + j;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * nt + 4 * kk + r, n = n0 + row;
                const float v = acc[nt][r];
                if (MODE == MS_FWD) {
                    float c = 0.f;
                    if (n < p.N) {
                        c = lrelu(v + p.g[(qrow + n) * Hp + col]);
                        if (p.c != nullptr) p.c[(qrow + n) * Hp + col] = c;
                    }
                    Cl[row * CP + col] = c;
                } else if (n < p.N) {
                    if (MODE == MS_BWD_PRE) {
                        const size_t i = (srow + n) * Hp + col;
                        p.dpre[(qrow + n) * Hp + col] = v * lrelu_grad_from_out(p.c[(qrow + n) * Hp + col]);
                        const float d = Ml[row * MP + col];
#pragma unroll
                        for (int k = 0; k < MS_MAXK; ++k)                  // (unrolled: part[] stays in registers)
                            if (k < Kk) part[k] += d * (p.Hs[(size_t)(p.t + k) * slot + i] + p.R[((size_t)k * p.N + n) * Hp + col]);
                    } else {
                        const size_t i = (srow + n) * Hp + col;
                        const float d = p.dH[(size_t)(Kk + p.t) * slot + i], wv = p.w[(size_t)n * Hp + col];
                        for (int k = 0; k < Kk; ++k) {
                            float* o = p.dH + (size_t)(p.t + k) * slot + i;
                            *o += att[k] * d + dev[k] * wv + (k == Kk - 1 ? v : 0.f);
                        }
                    }
                }
            }
    }

    if (MODE == MS_BWD_PRE) {
#pragma unroll
        for (int k = 0; k < MS_MAXK; ++k) {
            if (k >= Kk) break;                                          // (uniform)
            const float s = ms_block_sum(part[k], red, tid);
            if (tid == 0) p.pa[((size_t)b * p.G + blockIdx.x) * MS_MAXK + k] = s;
        }
    }
    if (MODE == MS_FWD) {
        // ---- o = c W2^T + b + sum_k a_k (s_k + R_k), and this workgroup's share of w . o ----
        __syncthreads();
        float s1 = 0.f, s2 = 0.f;
        float* out = p.Hs + (size_t)(p.t + Kk) * slot;
        for (int ct = wave; 16 * ct < Hp; ct += RECUR_THREADS / 64) {
            f32x4 acc[NT];
            recur_gemm_tiles<NT>(acc, Cl, CP, p.W2, Hp, ct, j, kk);
            const int col = 16 * ct + j;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = n0 + 16 * nt + 4 * kk + r;
                    if (n >= p.N) continue;
                    const size_t i = (srow + n) * Hp + col, ni = (size_t)n * Hp + col;
                    float v = acc[nt][r] + p.bvec[ni];
                    for (int k = 0; k < Kk; ++k) v += att[k] * (p.Hs[(size_t)(p.t + k) * slot + i] + p.R[(size_t)k * p.N * Hp + ni]);
                    out[i] = v;
                    s1 += v * p.w[ni];
                    if (p.sig2 != nullptr) s2 += v * p.w2[ni];
                }
        }
        const size_t si = ((size_t)(p.t + Kk) * p.B + b) * p.G + blockIdx.x;
        s1 = ms_block_sum(s1, red, tid);
        if (tid == 0) p.sig[si] = s1;
        if (p.sig2 != nullptr) {
            s2 = ms_block_sum(s2, red, tid);
            if (tid == 0) p.sig2[si] = s2;
        }
    }
}

// ---- launch ----
static size_t ms_lds_bytes(int mode, int Np, int Hp, int ks, int nt) {
    const size_t slab = mode == MS_BWD_PRE ? 0 : (size_t)Np * RECUR_SP;
    const size_t K = mode == MS_BWD_PRE ? Hp : (size_t)(ks + 1) * Hp;
    return (slab + (size_t)16 * nt * (K + 4) + (mode == MS_FWD ? (size_t)16 * nt * (Hp + 4) : 0)) * sizeof(float);
}

static int ms_groups(int B, int Np, int forced) {
    const int nt = recur_tiles(B, Np, forced);
    return (Np / 16 + nt - 1) / nt;
}

template <int MODE>
static int ms_launch(MsStep p, int tiles, void* stream) {
    if (MODE != MS_BWD_PRE && (!p.L || p.ks < 1 || p.ks > 3)) return GPTST_EARG;
    const int rc = recur_check(p.Wt, p.B, p.T, p.N, p.t, tiles, p.Hp, p.Np);
    if (rc != GPTST_OK) return rc;
    if (p.Kk < 1 || p.Kk > MS_MAXK) return GPTST_ESHAPE;
    const int nt = recur_tiles(p.B, p.Np, tiles);
    p.G = ms_groups(p.B, p.Np, tiles);
    const size_t smem = ms_lds_bytes(MODE, p.Np, p.Hp, p.ks, nt);
    if (smem > RECUR_LDS_MAX) return GPTST_ESHAPE;
    return nt == 2 ? recur_launch<ms_step_kernel<MODE, 2>>(p, dim3(p.G, p.B), smem, (hipStream_t)stream)
                   : recur_launch<ms_step_kernel<MODE, 1>>(p, dim3(p.G, p.B), smem, (hipStream_t)stream);
}

extern "C" int gptst_msdr_lds_bytes(int N, int Hp, int B, int ks) {
    if (N <= 0 || Hp <= 0 || B <= 0 || ks < 1) return GPTST_EARG;
    const int Np = 16 * ((N + 15) / 16);
    return (int)ms_lds_bytes(MS_FWD, Np, Hp, ks, recur_tiles(B, Np, 0));      // the widest of the three launches
}

extern "C" int gptst_msdr_groups(int N, int B, int tiles) {
    if (N <= 0 || B <= 0 || tiles < 0 || tiles > 2) return GPTST_EARG;
    return ms_groups(B, 16 * ((N + 15) / 16), tiles);
}

extern "C" int gptst_msdr_fwd_step(const float* L, int Np, int ks, const float* Wh, const float* W2, const float* bvec, const float* R,
                                   const float* w, const float* w2, const float* wr, const float* Gx, float* Hs, float* sig, float* sig2,
                                   float* c, float* z, int ldz, float* a, int B, int T, int N, int Hp, int Kk, int t, int tiles, void* stream) {
    if (!W2 || !bvec || !R || !w || !wr || !Gx || !Hs || !sig || (sig2 != nullptr) != (w2 != nullptr)) return GPTST_EARG;
    if (z != nullptr && (ldz != (ks + 1) * Hp)) return GPTST_EARG;
    MsStep p{};
    p.L = L; p.Np = Np; p.ks = ks; p.Wt = Wh; p.NO = Hp; p.K = (ks + 1) * Hp; p.W2 = W2; p.B = B; p.T = T; p.N = N; p.Hp = Hp; p.t = t; p.Kk = Kk;
    p.g = Gx; p.bvec = bvec; p.R = R; p.w = w; p.w2 = w2; p.wr = wr; p.Hs = Hs; p.sig = sig; p.sig2 = sig2; p.c = c; p.z = z; p.ldz = ldz; p.a = a;
    return ms_launch<MS_FWD>(p, tiles, stream);
}

extern "C" int gptst_msdr_bwd_pre(const float* W, const float* R, const float* Hs, const float* dH, const float* c, float* dpre, float* pa,
                                  int B, int T, int N, int Hp, int Kk, int t, int tiles, void* stream) {
    if (!R || !Hs || !dH || !c || !dpre || !pa) return GPTST_EARG;
    MsStep p{};
    p.Np = 16 * ((N + 15) / 16); p.ks = 1; p.Wt = W; p.NO = Hp; p.K = Hp; p.B = B; p.T = T; p.N = N; p.Hp = Hp; p.t = t; p.Kk = Kk;
    p.R = R; p.Hs = const_cast<float*>(Hs); p.dH = const_cast<float*>(dH); p.c = const_cast<float*>(c); p.dpre = dpre; p.pa = pa;
    return ms_launch<MS_BWD_PRE>(p, tiles, stream);
}

extern "C" int gptst_msdr_bwd_state(const float* LT, int Np, int ks, const float* WhT, const float* w, const float* a, const float* pa,
                                    const float* dpre, float* dH, float* de, int B, int T, int N, int Hp, int Kk, int t, int tiles,
                                    void* stream) {
    if (!w || !a || !pa || !dpre || !dH || !de) return GPTST_EARG;
    MsStep p{};
    p.L = LT; p.Np = Np; p.ks = ks; p.Wt = WhT; p.NO = Hp; p.K = (ks + 1) * Hp; p.B = B; p.T = T; p.N = N; p.Hp = Hp; p.t = t; p.Kk = Kk;
    p.w = w; p.a = const_cast<float*>(a); p.pa = const_cast<float*>(pa); p.dpre = const_cast<float*>(dpre); p.dH = dH; p.de = de;
    return ms_launch<MS_BWD_STATE>(p, tiles, stream);
}
