// The stacked LSTM of the downstream ST-MGCN predictor (reference model/STMGCN_demand/STMGCN.py:19-20,45-48; gpt-st_amd/predictors/stmgcn.py) on HIP,
// forward and backward, each ONE launch for all T steps of all L layers.  An LSTM row (b, n) reads no other row, so nothing has to cross a
// workgroup between two steps (TGCN and MSDR mix the nodes inside the step and take a launch per step: tgcn.hip, msdr.hip): a workgroup of
// RECUR_THREADS owns NT 16-row tiles, keeps every layer's h and c (backward: the dh and dc carries) in LDS and reads the weights from L2.
//
//   forward, t = 0 .. T-1 outer, l = 0 .. L-1 inner
//     pre = [h_{l-1,t} | h_{l,t-1}] W_l^T + b_l        (layer 0: h_{0,t-1} W_hh0^T + Gx0[t], the input half hoisted with both biases)
//     i, f, o = sigmoid, g = tanh of the four H-wide blocks of pre (torch's order i, f, g, o);  c = f c_prev + i g;  h = o tanh(c)
//   backward, t = T-1 .. 0 outer, l = L-1 .. 0 inner
//     dh = (top layer: dTop[t];  else layer l+1's dx) + the carry of step t+1;  dc = dh o (1 - tanh(c)^2) + the dc carry
//     dG = [dc g i(1-i) | dc c_prev f(1-f) | dc i (1-g^2) | dh tanh(c) o(1-o)];  dc carry = dc f;  [dx | dh carry] = dG W_l
//
// The GEMM is recur_gemm_tiles (recur_step_dev.h): wave w owns channel tiles w, w + 4 of the H channels and runs the loop once per gate
// block, on column tiles c, c + H/16, c + 2H/16, c + 3H/16 of W_l — at H = 64 tiles w, w + 4, w + 8, w + 12 — so the four gates of a (row,
// channel) land in the same lane's accumulators at any H without reordering the weights, and no gate meets its siblings through LDS or HBM.
// A row's state depends on its own row only: the rows past `rows` of a half-filled tile compute on zeros and are never stored.
// Weight gradients are not formed here: dG and the h ring are contiguous (T rows, width) operands of gptst_stgcn_wgrad.
// fp32 MFMA 16x16x4 (exact fp32); plain launches, no workgroup waits on another, no float atomics: two runs are bit-equal.
#include "common.h"
#include "gptst_hip.h"
#include "recur_step_dev.h"

#define ST_MAXL 4
#define ST_MAXT 32

struct StLstm {
    int rows, T, L, H;
    // forward
    const float* Gx0;              // (T, rows, 4H)
    const float* W;                // W_0 (4H, H) then W_l (4H, 2H), l = 1 .. L-1, one after the other
    const float* bias;             // (L, 4H); row 0 is not read
    float* top;                    // (T, rows, H): written when nothing is kept
    float *Gk, *Ck, *Hr;           // kept: gates (L, T, rows, 4H), c (L, T, rows, H), h (L, T + 1, rows, H) slot 0 = 0 (the caller's)
    // backward
    const float* dTop;             // (T, rows, H)
    const float* WT;               // W_0^T (H, 4H) then W_l^T (2H, 4H)
    float* dG; int dGL;            // (dGL, T, rows, 4H): layers 0 .. dGL - 1 are written
};

__device__ __forceinline__ size_t st_woff(int l, int H) { return l == 0 ? 0 : (size_t)4 * H * H + (size_t)(l - 1) * 8 * H * H; }

template <int NT>
__global__ __launch_bounds__(RECUR_THREADS) void st_lstm_fwd_kernel(StLstm p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = 16 * NT;
    const int H = p.H, L = p.L, HT = H / 16, P = 2 * H + 4;
    float* A = smem;                                 // [L][R][P]: row = [h_{l-1,t} | h_{l,t-1}], the A operand of layer l's GEMM
    float* Cs = smem + (size_t)L * R * P;            // [L][R][H]: c_l
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int row0 = blockIdx.x * R;
    for (int f = tid; f < L * R * (P + H); f += RECUR_THREADS) smem[f] = 0.f;      // the zero initial state
    __syncthreads();
    for (int t = 0; t < p.T; ++t)
        for (int l = 0; l < L; ++l) {
            const int K = l ? 2 * H : H;
            const float* Al = A + (size_t)l * R * P + (l ? 0 : H);
            const float* Wl = p.W + st_woff(l, H);
            float hreg[2][NT][4];
#pragma unroll
            for (int ci = 0; ci < 2; ++ci) {
                const int c = wave + 4 * ci;                               // (wave-uniform)
                if (c < HT) {
                    f32x4 acc[4][NT];
#pragma unroll
                    for (int g = 0; g < 4; ++g) recur_gemm_tiles<NT>(acc[g], Al, P, Wl, K, c + g * HT, j, kk);
                    const int col = 16 * c + j;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * nt + 4 * kk + r;
                            const size_t grow = (size_t)row0 + row;
                            const bool valid = grow < (size_t)p.rows;
                            float b[4];
#pragma unroll
                            for (int g = 0; g < 4; ++g)
                                b[g] = l ? p.bias[(size_t)l * 4 * H + g * H + col]
                                         : (valid ? p.Gx0[((size_t)t * p.rows + grow) * 4 * H + g * H + col] : 0.f);
                            const float gi = sigmoidf_(acc[0][nt][r] + b[0]), gf = sigmoidf_(acc[1][nt][r] + b[1]);
                            const float gg = tanhf(acc[2][nt][r] + b[2]), go = sigmoidf_(acc[3][nt][r] + b[3]);
                            float* cp = Cs + ((size_t)l * R + row) * H + col;
                            const float cn = gf * *cp + gi * gg, h = go * tanhf(cn);
                            *cp = cn;
                            hreg[ci][nt][r] = h;
                            if (!valid) continue;
                            if (p.Gk != nullptr) {
                                const size_t u = ((size_t)l * p.T + t) * p.rows + grow;
                                float* gk = p.Gk + u * 4 * H + col;
                                gk[0] = gi; gk[H] = gf; gk[2 * H] = gg; gk[3 * H] = go;
                                p.Ck[u * H + col] = cn;
                                p.Hr[(((size_t)l * (p.T + 1) + t + 1) * p.rows + grow) * H + col] = h;
                            } else if (l == L - 1) {
                                p.top[((size_t)t * p.rows + grow) * H + col] = h;
                            }
                        }
                }
            }
            __syncthreads();                                               // every wave has read layer l's operand
#pragma unroll
            for (int ci = 0; ci < 2; ++ci) {
                const int c = wave + 4 * ci;
                if (c < HT) {
                    const int col = 16 * c + j;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = 16 * nt + 4 * kk + r;
                            A[((size_t)l * R + row) * P + H + col] = hreg[ci][nt][r];                        // h_{l,t}: its own next step
                            if (l + 1 < L) A[((size_t)(l + 1) * R + row) * P + col] = hreg[ci][nt][r];       // and layer l + 1's input
                        }
                }
            }
            __syncthreads();
        }
}

template <int NT>
__global__ __launch_bounds__(RECUR_THREADS) void st_lstm_bwd_kernel(StLstm p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = 16 * NT;
    const int H = p.H, L = p.L, T = p.T, P = 4 * H + 4;
    float* dhc = smem;                               // [L][R][H]: the gradient of h_{l,t} that step t + 1 left
    float* dcc = dhc + (size_t)L * R * H;            // [L][R][H]: the same of c_{l,t}
    float* dxb = dcc + (size_t)L * R * H;            // [R][H]: layer l + 1's dx
    float* dGb = dxb + (size_t)R * H;                // [R][P]: dG of the layer at hand, the A operand of its GEMM
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kk = lane >> 4;
    const int row0 = blockIdx.x * R;
    for (int f = tid; f < 2 * L * R * H; f += RECUR_THREADS) smem[f] = 0.f;
    __syncthreads();
    for (int t = T - 1; t >= 0; --t)
        for (int l = L - 1; l >= 0; --l) {
            for (int f = tid; f < R * H; f += RECUR_THREADS) {
                const int row = f / H, col = f - row * H;
                const size_t grow = (size_t)row0 + row;
                float d[4] = {0.f, 0.f, 0.f, 0.f};
                if (grow < (size_t)p.rows) {
                    const size_t s = (size_t)l * R * H + f, u = ((size_t)l * T + t) * p.rows + grow;
                    const float dh = (l == L - 1 ? p.dTop[((size_t)t * p.rows + grow) * H + col] : dxb[f]) + dhc[s];
                    const float* gk = p.Gk + u * 4 * H + col;
                    const float gi = gk[0], gf = gk[H], gg = gk[2 * H], go = gk[3 * H];
                    const float tc = tanhf(p.Ck[u * H + col]);
                    const float cprev = t ? p.Ck[(u - p.rows) * H + col] : 0.f;
                    const float dc = dh * go * (1.f - tc * tc) + dcc[s];
                    dcc[s] = dc * gf;
                    d[0] = dc * gg * (gi * (1.f - gi));
                    d[1] = dc * cprev * (gf * (1.f - gf));
                    d[2] = dc * gi * (1.f - gg * gg);
                    d[3] = dh * tc * (go * (1.f - go));
                    if (l < p.dGL) {
                        float* o = p.dG + u * 4 * H + col;
                        o[0] = d[0]; o[H] = d[1]; o[2 * H] = d[2]; o[3 * H] = d[3];
                    }
                }
                float* o = dGb + (size_t)row * P + col;
                o[0] = d[0]; o[H] = d[1]; o[2 * H] = d[2]; o[3 * H] = d[3];
            }
            __syncthreads();
            const int NO = l ? 2 * H : H;
            const float* WTl = p.WT + st_woff(l, H);
            for (int ct = wave; 16 * ct < NO; ct += RECUR_THREADS / 64) {
                f32x4 acc[NT];
                recur_gemm_tiles<NT>(acc, dGb, P, WTl, 4 * H, ct, j, kk);
                const int col = 16 * ct + j;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * nt + 4 * kk + r;
                        if (l && col < H) dxb[row * H + col] = acc[nt][r];
                        else dhc[((size_t)l * R + row) * H + col - (l ? H : 0)] = acc[nt][r];
                    }
            }
            __syncthreads();
        }
}

// ---- launch ----
static size_t st_lds_fwd(int H, int L, int nt) { return (size_t)L * 16 * nt * (3 * H + 4) * sizeof(float); }
static size_t st_lds_bwd(int H, int L, int nt) { return (size_t)16 * nt * (2 * L * H + 5 * H + 4) * sizeof(float); }
static size_t st_lds(int H, int L, int nt) { const size_t a = st_lds_fwd(H, L, nt), b = st_lds_bwd(H, L, nt); return a > b ? a : b; }

// row tiles per workgroup, the same forward and backward: 2 while that still leaves more workgroups than the chip has CUs and both launches'
// LDS fits, else 1
static int st_tiles(int rows, int H, int L, int forced) {
    if (forced == 1 || forced == 2) return forced;
    const long tiles = ((long)rows + 15) / 16;
    return (tiles + 1) / 2 > 256 && st_lds(H, L, 2) <= RECUR_LDS_MAX ? 2 : 1;
}

static int st_check(int rows, int T, int L, int H, int tiles) {
    if (rows <= 0 || T <= 0 || L <= 0 || tiles < 0 || tiles > 2) return GPTST_EARG;
    if (H < 16 || H > 128 || H % 16 || L > ST_MAXL || T > ST_MAXT || ((long)rows + 15) / 16 > 0x7fffffffL / 2) return GPTST_ESHAPE;
    return GPTST_OK;
}

extern "C" int gptst_stmgcn_lds_bytes(int H, int L, int tiles) {
    if (H <= 0 || L <= 0 || tiles < 1 || tiles > 2) return GPTST_EARG;
    return (int)st_lds(H, L, tiles);
}

extern "C" int gptst_stmgcn_tiles(int rows, int H, int L, int forced) {
    const int rc = st_check(rows, 1, L, H, forced);
    return rc != GPTST_OK ? rc : st_tiles(rows, H, L, forced);
}

extern "C" int gptst_stmgcn_lstm_fwd(const float* Gx0, const float* W, const float* bias, float* top, float* gates, float* c, float* h, int rows,
                                     int T, int L, int H, int tiles, void* stream) {
    const bool keep = gates != nullptr;
    if (!Gx0 || !W || !bias || keep != (c != nullptr) || keep != (h != nullptr) || keep == (top != nullptr)) return GPTST_EARG;
    const int rc = st_check(rows, T, L, H, tiles);
    if (rc != GPTST_OK) return rc;
    const int nt = st_tiles(rows, H, L, tiles);
    const size_t smem = st_lds_fwd(H, L, nt);
    if (st_lds(H, L, nt) > RECUR_LDS_MAX) return GPTST_ESHAPE;
    StLstm p{};
    p.rows = rows; p.T = T; p.L = L; p.H = H; p.Gx0 = Gx0; p.W = W; p.bias = bias; p.top = top; p.Gk = gates; p.Ck = c; p.Hr = h;
    const dim3 grid((unsigned)(((long)rows + 16 * nt - 1) / (16 * nt)));
    return nt == 2 ? recur_launch<st_lstm_fwd_kernel<2>>(p, grid, smem, (hipStream_t)stream)
                   : recur_launch<st_lstm_fwd_kernel<1>>(p, grid, smem, (hipStream_t)stream);
}

extern "C" int gptst_stmgcn_lstm_bwd(const float* dTop, const float* WT, const float* gates, const float* c, float* dG, int dG_layers, int rows,
                                     int T, int L, int H, int tiles, void* stream) {
    if (!dTop || !WT || !gates || !c || !dG || dG_layers < 1 || dG_layers > L) return GPTST_EARG;
    const int rc = st_check(rows, T, L, H, tiles);
    if (rc != GPTST_OK) return rc;
    const int nt = st_tiles(rows, H, L, tiles);
    const size_t smem = st_lds_bwd(H, L, nt);
    if (st_lds(H, L, nt) > RECUR_LDS_MAX) return GPTST_ESHAPE;
    StLstm p{};
    p.rows = rows; p.T = T; p.L = L; p.H = H; p.dTop = dTop; p.WT = WT; p.Gk = const_cast<float*>(gates); p.Ck = const_cast<float*>(c);
    p.dG = dG; p.dGL = dG_layers;
    const dim3 grid((unsigned)(((long)rows + 16 * nt - 1) / (16 * nt)));
    return nt == 2 ? recur_launch<st_lstm_bwd_kernel<2>>(p, grid, smem, (hipStream_t)stream)
                   : recur_launch<st_lstm_bwd_kernel<1>>(p, grid, smem, (hipStream_t)stream);
}
