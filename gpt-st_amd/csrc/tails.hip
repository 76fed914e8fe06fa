// Fused "thin head" kernels at the two places where the loss meets the network — one pass over the C-wide activation each,
// replacing chains of 4-6 small launches:
//
//   mae tail  (reference GPTST.py:455 dim_flow_out, Run.py:92-100 scaler_mae_loss, lib/metrics.py:11-18 and their autograd backward)
//       out = dec W^T + b;  p = (out s + m) M, y = (label s + m) M, keep = y > thresh;  stats += (sum_keep |y-p|, #keep);
//       a = sign(p-y) M s [keep]  (gradient of the SUM loss: the 1/#keep of the mean is applied by the optimiser, hyper[9] = 1);
//       d_dec = a W;  partial (gW, gb) = (a^T dec, sum a)                    was rowdot, mae_fwd, mae_bwd, lin_in, rowouter x2
//   kl head   (reference BasicTrainer.py:85 0.1 KLDivLoss(sum)(log prob, eb), softmax + MLP_RL.ln3 GPTST.py:33 backward)
//       a = w (prob sum_h eb - eb);  stats[2] += sum eb (log eb - log prob);  d_h2 = a W3;  partial (gW3, gb3) = (a^T h2, sum a)
//                                                                          was kl, lin_in, rowouter x2
// Layout as small.hip: C/4 lanes per row (float4 columns), 16 row slots per workgroup; TL_NB persistent workgroups walk contiguous
// row chunks, keep the weight-gradient partials in registers and fold them through LDS once at the end: part[blk][J*C + J]
// (the caller sums the TL_NB partials of [gW | gb] with one bwd_pool job) and write their loss statistics to sws[blk][4]
// ([0] sum |y-p|, [1] kept count: mae tail; [2] KL sum: kl head), which gptst_stats_fold sums in index order into stats: no float
// atomics, the result does not depend on scheduling.  (Measured: 510 same-address atomics at the end of a launch — the stats
// themselves, or a "last workgroup folds" ticket — cost ~8 us; one extra 1-workgroup launch costs 2.5.)
// C in {64, 128}, J <= TL_MAXJ; other shapes use the unfused ops.
#include "kl_guest.h"         // TailArgs, tail_mfma_body (the KL head also runs as a guest of the hyperTem forward chain)

#define TL_NB 512

template <int KIND, int C>      // KIND 0: mae tail, 1: kl head
__global__ __launch_bounds__(256) void tail_kernel(TailArgs t) {
    constexpr int LPR = C / 4, RPB = 256 / LPR;
    __shared__ __attribute__((aligned(16))) float Ws[TL_MAXJ * C];
    __shared__ float4 red[RPB][LPR];
    __shared__ float redb[RPB];
    __shared__ float reds[3][4];
    const int J = t.J;
    for (int i = threadIdx.x; i < J * C / 4; i += 256) st4(Ws + 4 * i, ld4(t.W + 4 * i));
    __syncthreads();
    const int c4 = threadIdx.x % LPR, slot = threadIdx.x / LPR;
    const size_t r0 = (size_t)blockIdx.x * t.rows_per_block;
    const size_t r1 = min((size_t)t.rows, r0 + t.rows_per_block);
    float4 accW[TL_MAXJ];
    float accb[TL_MAXJ];
#pragma unroll
    for (int j = 0; j < TL_MAXJ; ++j) { accW[j] = f4zero(); accb[j] = 0.f; }
    float s0 = 0.f, s1 = 0.f;                                         // mae: sum |y-p|, count;  kl: sum, -
    constexpr int UR = 4;                                             // independent rows in flight per thread
    for (size_t i0 = r0 + slot; i0 < r1; i0 += UR * RPB) {
      float4 xs[UR];
#pragma unroll
      for (int u = 0; u < UR; ++u) { const size_t i = i0 + (size_t)u * RPB; xs[u] = i < r1 ? ld4(t.X + i * C + 4 * c4) : f4zero(); }
      SB();
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const size_t i = i0 + (size_t)u * RPB;
        if (i >= r1) continue;                                        // uniform per 16-lane row group; no barrier inside
        const float4 x = xs[u];
        // per-row scalars: lane j of the row's C/4-lane group loads / computes entry j (J <= 16) and the group shares the results —
        // every lane loading all J entries itself cost 16x the load instructions (42 us for the KL head at the bench shape)
        float a[TL_MAXJ];
        float a_own = 0.f;
        const int gl = (threadIdx.x & 63) & ~(LPR - 1);                // first lane of this row group within the wave
        if (KIND == 0) {
            float o_all[TL_MAXJ];
#pragma unroll
            for (int j = 0; j < TL_MAXJ; ++j) {
                o_all[j] = 0.f;
                if (j < J) o_all[j] = group_sum<LPR>(f4dot(x, ld4(Ws + j * C + 4 * c4)));      // uniform branch
            }
            float o = 0.f;
#pragma unroll
            for (int j = 0; j < TL_MAXJ; ++j) if (j == c4) o = o_all[j];
            if (c4 < J) {
                o += t.b ? t.b[c4] : 0.f;
                const size_t e = i * J + c4;
                const float M = 1.f - t.mask[e];
                const float p = inverse_transform(o, t.sigma, t.mu) * M;
                const float y = inverse_transform(t.src[i * t.lda + c4], t.sigma, t.mu) * M;
                if (y > t.thresh) {
                    const float d = p - y;
                    s0 += fabsf(d); s1 += 1.f;
                    a_own = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) * M * t.sigma;
                }
                t.out[e] = o;
            }
        } else {
            const size_t bt = i / t.N, n = i % t.N;
            float e_ = 0.f, p_ = 1.f;
            if (c4 < J) { e_ = t.c[(bt * J + c4) * t.N + n]; p_ = t.prob[i * J + c4]; }
            const float se = group_sum<LPR>(e_);
            if (c4 < J && e_ > 0.f) s0 += e_ * (logf(e_) - logf(p_));
            a_own = c4 < J ? t.w * (p_ * se - e_) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < TL_MAXJ; ++j) a[j] = j < J ? __shfl(a_own, gl + j, 64) : 0.f;
        float4 dx = f4zero();
#pragma unroll
        for (int j = 0; j < TL_MAXJ; ++j)
            if (j < J) {
                dx = f4fma(a[j], ld4(Ws + j * C + 4 * c4), dx);
                accW[j] = f4fma(a[j], x, accW[j]);
                accb[j] += a[j];
            }
        if (t.premul) {
            dx.x *= lrelu_grad_from_out(x.x); dx.y *= lrelu_grad_from_out(x.y); dx.z *= lrelu_grad_from_out(x.z); dx.w *= lrelu_grad_from_out(x.w);
        }
        st4(t.dX + i * C + 4 * c4, dx);
      }
    }
    // ---- fold the 16 row slots of the workgroup, then the loss statistics ----
    float* mine = t.part + (size_t)blockIdx.x * (J * C + J);
#pragma unroll
    for (int j = 0; j < TL_MAXJ; ++j) {
        if (j >= J) continue;                                         // uniform
        red[slot][c4] = accW[j];
        if (c4 == 0) redb[slot] = accb[j];
        __syncthreads();
        if (slot == 0) {
            float4 s = red[0][c4];
            for (int q = 1; q < RPB; ++q) s = f4add(s, red[q][c4]);
            st4(mine + j * C + 4 * c4, s);
            if (c4 == 0) {
                float sb = redb[0];
                for (int q = 1; q < RPB; ++q) sb += redb[q];
                mine[J * C + j] = sb;
            }
        }
        __syncthreads();
    }
    s0 = group_sum<64>(s0); s1 = group_sum<64>(s1);
    if ((threadIdx.x & 63) == 0) { reds[0][threadIdx.x >> 6] = s0; reds[1][threadIdx.x >> 6] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* w = t.sws + 4 * (size_t)blockIdx.x;
        const float v0 = (reds[0][0] + reds[0][1]) + (reds[0][2] + reds[0][3]), v1 = (reds[1][0] + reds[1][1]) + (reds[1][2] + reds[1][3]);
        if (KIND == 0) { w[0] = v0; w[1] = v1; } else { w[2] = v0; }
    }
}

// ---- the same two heads on MFMA 16x16x4 (C = 64, r03): kl_guest.h, tail_mfma_body --------------------------------------------------------
template <int KIND, int C>
__global__ __launch_bounds__(256) void tail_mfma_kernel(TailArgs t) {
    __shared__ __attribute__((aligned(16))) float lds[tail_mfma_lds_floats<C>()];
    tail_mfma_body<KIND, C>(t, blockIdx.x, lds);
}

// stats[k] += sum over rows of sws[row][k], k < 3, in a fixed order (thread t: rows t, t+256, ...; then a fixed tree)
// lost0 / lost1 (may be NULL): the hand-off expiry counters — their sum goes to stats[5], so that a gradient all-reduce carries it to every rank and
// all of them skip the update together (gptst_clip_adam's guard)
__global__ __launch_bounds__(256) void stats_fold_kernel(const float* __restrict__ sws, int rows, float* __restrict__ stats,
                                                         const unsigned* __restrict__ lost0, const unsigned* __restrict__ lost1,
                                                         const unsigned* __restrict__ lost2) {
    __shared__ float red[3][4];
    if (threadIdx.x == 255) stats[5] = (float)((lost0 != nullptr ? *lost0 : 0u) + (lost1 != nullptr ? *lost1 : 0u) + (lost2 != nullptr ? *lost2 : 0u));
    float s[3] = {0.f, 0.f, 0.f};
    for (int r = threadIdx.x; r < rows; r += 256) {
        const float4 v = ld4(sws + 4 * (size_t)r);
        s[0] += v.x; s[1] += v.y; s[2] += v.z;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s[k] = group_sum<64>(s[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) stats[threadIdx.x] += (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

thread_local int g_tl_nb = TL_NB;       // experiments: gptst_tune(6, nb)
thread_local int g_tl_mfma = 1;         // gptst_tune(15, 0): the VALU loss heads (tail_kernel) instead of the MFMA ones
static void tl_geometry(int rows, int& nb, int& rpb) {
    int want = g_tl_nb;
    if (g_tl_nb == TL_NB && rows > TL_NB * 512) { want = rows / 512; if (want > 4096) want = 4096; }      // N = 4096: 1.5 M rows -> 3072 chunks
    rpb = (rows + want - 1) / want; if (rpb < 16) rpb = 16;
    nb = (rows + rpb - 1) / rpb;
}

// number of row-chunk partials that gptst_tail_mae / gptst_tail_kl write: part must hold that many x (J*C + J) floats
extern "C" int gptst_tail_parts(int rows) { int nb, rpb; tl_geometry(rows, nb, rpb); return nb; }
// ... and the rows per chunk, for a launch that carries the KL head as guests
GPTST_INTERNAL int gptst_tail_geometry(int rows, int* rows_per_block) { int nb; tl_geometry(rows, nb, *rows_per_block); return nb; }

GPTST_INTERNAL const unsigned* gptst_handoff_word_capmfma(void);
GPTST_INTERNAL const unsigned* gptst_handoff_word_hypertem(void);
GPTST_INTERNAL const unsigned* gptst_handoff_word_masksel(void);
// sum the per-workgroup loss statistics sws (rows, 4) of the tail kernels into stats[0..2] (+=), in a fixed order; stats[5] <- hand-off expiries on record
extern "C" int gptst_stats_fold(const float* sws, int rows, float* stats, void* stream) {
    if (!sws || !stats || rows <= 0) return GPTST_EARG;
    static const unsigned* w0 = gptst_handoff_word_capmfma();         // looked up once (the steppers warm up before any capture)
    static const unsigned* w1 = gptst_handoff_word_hypertem();
    static const unsigned* w2 = gptst_handoff_word_masksel();
    hipLaunchKernelGGL(stats_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sws, rows, stats, w0, w1, w2);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_tail_mae(const float* dec, const float* W, const float* b, const float* src, int lda, const float* mask, float sigma,
                              float mu, float thresh, float* out, float* d_dec, float* part, float* sws, int premul, int rows, int J, int C,
                              void* stream) {
    if (!dec || !W || !src || !mask || !out || !d_dec || !part || !sws || rows <= 0 || J <= 0) return GPTST_EARG;
    if ((C != 64 && C != 128) || J > TL_MAXJ) return GPTST_ESHAPE;
    TailArgs t{};
    t.X = dec; t.W = W; t.b = b; t.dX = d_dec; t.part = part; t.sws = sws; t.rows = rows; t.J = J;
    t.src = src; t.mask = mask; t.out = out; t.lda = lda; t.sigma = sigma; t.mu = mu; t.thresh = thresh; t.premul = premul;
    int nb; tl_geometry(rows, nb, t.rows_per_block);
    if (C == 64 && g_tl_mfma) hipLaunchKernelGGL((tail_mfma_kernel<0, 64>), dim3(nb), dim3(256), 0, (hipStream_t)stream, t);
    else if (C == 64) hipLaunchKernelGGL((tail_kernel<0, 64>), dim3(nb), dim3(256), 0, (hipStream_t)stream, t);
    else if (g_tl_mfma) hipLaunchKernelGGL((tail_mfma_kernel<0, 128>), dim3(nb), dim3(256), 0, (hipStream_t)stream, t);
    else hipLaunchKernelGGL((tail_kernel<0, 128>), dim3(nb), dim3(256), 0, (hipStream_t)stream, t);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_tail_kl(const float* h2, const float* W3, const float* prob, const float* c, float w, float* d_h2, float* part,
                             float* sws, int premul, int rows, int N, int HS, int C, void* stream) {
    if (!h2 || !W3 || !prob || !c || !d_h2 || !part || !sws || rows <= 0 || HS <= 0 || N <= 0) return GPTST_EARG;
    if ((C != 64 && C != 128) || HS > TL_MAXJ) return GPTST_ESHAPE;
    TailArgs t{};
    t.X = h2; t.W = W3; t.dX = d_h2; t.part = part; t.sws = sws; t.rows = rows; t.J = HS;
    t.prob = prob; t.c = c; t.N = N; t.w = w; t.premul = premul;
    int nb; tl_geometry(rows, nb, t.rows_per_block);
    if (C == 64 && g_tl_mfma) hipLaunchKernelGGL((tail_mfma_kernel<1, 64>), dim3(nb), dim3(256), 0, (hipStream_t)stream, t);
    else if (C == 64) hipLaunchKernelGGL((tail_kernel<1, 64>), dim3(nb), dim3(256), 0, (hipStream_t)stream, t);
    else if (g_tl_mfma) hipLaunchKernelGGL((tail_mfma_kernel<1, 128>), dim3(nb), dim3(256), 0, (hipStream_t)stream, t);
    else hipLaunchKernelGGL((tail_kernel<1, 128>), dim3(nb), dim3(256), 0, (hipStream_t)stream, t);
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}
