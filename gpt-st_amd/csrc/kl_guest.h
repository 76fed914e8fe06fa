// The KL term's backward through the guide classifier (BasicTrainer.py:85 0.1 KLDivLoss, GPTST.py:21-33) as __device__ bodies, so that its
// three launches can also run as GUEST workgroups appended to the grid of an earlier, one-round launch (gptst_hypertem_chain_fwd_kl):
//   stage 1  tail_mfma_body<1, C>      0.1 KL + softmax / ln3 backward -> d_h2                      (tails.hip, tail_mfma_kernel)
//   stage 2  applywg64_body<0, 2>      the time-conditioned layer (GPTST.py:29-32) -> d_h1, [dW|db]  (apply.hip, applywg64_kernel)
//   stage 3  guide_in_bwd_body<C>      node layer + ln1 on the low-rank form (GPTST.py:21-27)        (guidein.hip, guide_in_bwd_kernel)
// Each standalone kernel calls its body with blockIdx and a static LDS array; a host passes a virtual block id and its own dynamic LDS,
// so both forms run one code path and write bit-identical results.  The bodies take their LDS as a pointer because static __shared__ of a
// guest would be added to the host's own footprint on every workgroup of the launch.
#pragma once
#include "mfma_tile.h"
#include "wgrad64.h"

#define TL_MAXJ 16

struct TailArgs {
    const float* X; const float* W; const float* b; float* dX; float* part; float* sws;
    int rows, J, rows_per_block;
    // mae tail
    const float* src; const float* mask; float* out; int lda; float sigma, mu, thresh;
    // kl head
    const float* prob; const float* c; int N; float w;
    int premul;          // dPre chain: dX is multiplied by lrelu'(X) (X = the output of a LeakyReLU layer), include/gptst_hip.h
};

// ---- the loss heads on MFMA 16x16x4 (tails.hip, r03) ------------------------------------------------------------------------------------
// tail_kernel spends its time in J dot products per row (4 FMAs + a 4-step DPP reduction each), J rank-1 updates of the data gradient and J
// of the weight gradient per row.  Here a wave takes 16-row tiles and the three products are matrix products with register operands:
//   Z  (16 rows x 16 classes) = X . W^T          A = X rows straight from global (lane (j,kk): row j, channels 16q+4kk..), B = W[class j][..]
//   dX (16 rows x 64)         = a . W            A = a through a wave-private LDS tile (D layout -> A layout), B = W[class][4j+ct] (float4)
//   gW (16 classes x 64)     += a^T . X          A = a in the D layout as it is (step s <-> row 4kk+s), B = X rows in the D layout (float4)
// D layout of Z / a: lane (j = class, kk), register r <-> row 4kk + r, so the per-row softmax terms run across the 16 lanes of a DPP row.
// Same outputs as tail_kernel (out, dX, part[blk][J*C + J], sws[blk][4]); sums are accumulated in a different order (tolerance-checked).
// LDS (floats): fold [4][16 C + 16] | at [4][16][17] | reds [2][4]
template <int C>
constexpr int tail_mfma_lds_floats() { return 4 * (16 * C + 16) + 4 * 16 * 17 + 8; }

template <int KIND, int C>      // C = 128 (r05): the D-layout operands come in two 64-channel halves hf (channel 64 hf + 4j + ct)
__device__ __forceinline__ void tail_mfma_body(const TailArgs& t, int blk, float* __restrict__ lds) {
    constexpr int Q = C / 16, HF = C / 64;
    float (*fold)[16 * C + 16] = reinterpret_cast<float (*)[16 * C + 16]>(lds);
    float (*at)[16][17] = reinterpret_cast<float (*)[16][17]>(lds + 4 * (16 * C + 16));     // per wave: a[row][class] (D layout -> A layout)
    float (*reds)[4] = reinterpret_cast<float (*)[4]>(lds + 4 * (16 * C + 16) + 4 * 16 * 17);
    const int J = t.J;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, kk = lane >> 4;
    // W as B operand of Z (class j, channels 16q + 4kk ..) and of dX (class 4s + kk, channels 4j .. 4j+3)
    float4 bz[Q], bd[HF][4];
#pragma unroll
    for (int q = 0; q < Q; ++q) bz[q] = (KIND == 0 && j < J) ? ld4(t.W + (size_t)j * C + 16 * q + 4 * kk) : f4zero();
#pragma unroll
    for (int hf = 0; hf < HF; ++hf)
#pragma unroll
        for (int q = 0; q < 4; ++q) bd[hf][q] = (4 * q + kk < J) ? ld4(t.W + (size_t)(4 * q + kk) * C + 64 * hf + 4 * j) : f4zero();
    const float bj = (KIND == 0 && t.b != nullptr && j < J) ? t.b[j] : 0.f;
    const int nks = (J + 3) / 4;                        // k-steps of the dX product
    f32x4 gw[HF][4];
#pragma unroll
    for (int hf = 0; hf < HF; ++hf)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) gw[hf][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float gb = 0.f, s0 = 0.f, s1 = 0.f;
    const size_t r0 = (size_t)blk * t.rows_per_block;
    const size_t r1 = min((size_t)t.rows, r0 + t.rows_per_block);
    for (size_t tb = r0 + 16 * wave; tb < r1; tb += 64) {
        // X tile in both layouts (the second read hits L1): A layout for Z, D layout for gW / the LeakyReLU sign
        float4 xa[Q], xd[HF][4];
        if (KIND == 0) {
#pragma unroll
            for (int q = 0; q < Q; ++q) xa[q] = ld4(t.X + min(tb + j, r1 - 1) * C + 16 * q + 4 * kk);
        }
#pragma unroll
        for (int hf = 0; hf < HF; ++hf)
#pragma unroll
            for (int q = 0; q < 4; ++q) xd[hf][q] = ld4(t.X + min(tb + 4 * kk + q, r1 - 1) * C + 64 * hf + 4 * j);
        // the epilogue's per-row operands travel with the X tile (after the MFMAs they were a second, dependent round trip per tile)
        float o0[4], o1[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t i = min(tb + 4 * kk + r, r1 - 1);
            const int jc = min(j, J - 1);
            if (KIND == 0) { o0[r] = t.mask[i * J + jc]; o1[r] = t.src[i * t.lda + jc]; }
            else { const size_t bt = i / t.N, n = i % t.N; o0[r] = t.c[(bt * J + jc) * t.N + n]; o1[r] = t.prob[i * J + jc]; }
        }
        SB();
        float a[4];
        if (KIND == 0) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[q].x, bz[q].x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[q].y, bz[q].y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[q].z, bz[q].z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[q].w, bz[q].w, acc1, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t i = tb + 4 * kk + r;
                a[r] = 0.f;
                if (i < r1 && j < J) {
                    const float o = acc0[r] + acc1[r] + bj;
                    const size_t e = i * J + j;
                    const float M = 1.f - o0[r];
                    const float p = inverse_transform(o, t.sigma, t.mu) * M;
                    const float y = inverse_transform(o1[r], t.sigma, t.mu) * M;
                    if (y > t.thresh) {
                        const float d = p - y;
                        s0 += fabsf(d); s1 += 1.f;
                        a[r] = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) * M * t.sigma;
                    }
                    t.out[e] = o;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t i = tb + 4 * kk + r;
                const bool ok = i < r1 && j < J;
                float e_ = 0.f, p_ = 1.f;
                if (ok) { e_ = o0[r]; p_ = o1[r]; }
                const float se = group_sum<16>(e_);
                if (ok && e_ > 0.f) s0 += e_ * (logf(e_) - logf(p_));
                a[r] = ok ? t.w * (p_ * se - e_) : 0.f;
            }
        }
        // ---- gW += a^T X (step s <-> row 4kk + s on both operands), gb += column sums of a ----
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gb += a[r];
#pragma unroll
            for (int hf = 0; hf < HF; ++hf) {
                gw[hf][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], xd[hf][r].x, gw[hf][0], 0, 0, 0);
                gw[hf][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], xd[hf][r].y, gw[hf][1], 0, 0, 0);
                gw[hf][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], xd[hf][r].z, gw[hf][2], 0, 0, 0);
                gw[hf][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], xd[hf][r].w, gw[hf][3], 0, 0, 0);
            }
        }
        // ---- dX = a W: a from the D layout into the A layout (lane (i = row, kk): classes 4s + kk) through the wave's tile ----
#pragma unroll
        for (int r = 0; r < 4; ++r) at[wave][4 * kk + r][j] = a[r];
        f32x4 dx[HF][4];
#pragma unroll
        for (int hf = 0; hf < HF; ++hf)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) dx[hf][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s < nks) {                                           // uniform
                const float as = at[wave][j][4 * s + kk];
#pragma unroll
                for (int hf = 0; hf < HF; ++hf) {
                    dx[hf][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, bd[hf][s].x, dx[hf][0], 0, 0, 0);
                    dx[hf][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, bd[hf][s].y, dx[hf][1], 0, 0, 0);
                    dx[hf][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, bd[hf][s].z, dx[hf][2], 0, 0, 0);
                    dx[hf][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, bd[hf][s].w, dx[hf][3], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t i = tb + 4 * kk + r;
#pragma unroll
            for (int hf = 0; hf < HF; ++hf) {
                float4 v = make_float4(dx[hf][0][r], dx[hf][1][r], dx[hf][2][r], dx[hf][3][r]);
                if (t.premul) {
                    v.x *= lrelu_grad_from_out(xd[hf][r].x); v.y *= lrelu_grad_from_out(xd[hf][r].y);
                    v.z *= lrelu_grad_from_out(xd[hf][r].z); v.w *= lrelu_grad_from_out(xd[hf][r].w);
                }
                if (i < r1) st4(t.dX + i * C + 64 * hf + 4 * j, v);
            }
        }
    }
    // ---- fold the four waves: gW (D reg r of tile ct: class 4kk + r, channel 4j + ct), gb, loss statistics ----
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int hf = 0; hf < HF; ++hf) st4(&fold[wave][(4 * kk + r) * C + 64 * hf + 4 * j], make_float4(gw[hf][0][r], gw[hf][1][r], gw[hf][2][r], gw[hf][3][r]));
    gb += __shfl_xor(gb, 16, 64); gb += __shfl_xor(gb, 32, 64);
    if (kk == 0) fold[wave][16 * C + j] = gb;
    s0 = group_sum<64>(s0); s1 = group_sum<64>(s1);
    if (lane == 0) { reds[0][wave] = s0; reds[1][wave] = s1; }
    __syncthreads();
    float* mine = t.part + (size_t)blk * (J * C + J);
    for (int o = threadIdx.x; o < J * C; o += 256) mine[o] = (fold[0][o] + fold[1][o]) + (fold[2][o] + fold[3][o]);
    if ((int)threadIdx.x < J) mine[J * C + threadIdx.x] = (fold[0][16 * C + threadIdx.x] + fold[1][16 * C + threadIdx.x]) + (fold[2][16 * C + threadIdx.x] + fold[3][16 * C + threadIdx.x]);
    if (threadIdx.x == 0) {
        float* w = t.sws + 4 * (size_t)blk;
        const float v0 = (reds[0][0] + reds[0][1]) + (reds[0][2] + reds[0][3]), v1 = (reds[1][0] + reds[1][1]) + (reds[1][2] + reds[1][3]);
        if (KIND == 0) { w[0] = v0; w[1] = v1; } else { w[2] = v0; }
    }
}

// ---- fused backward of a generated-weight layer (apply.hip; see the comment above applywg64_kernel there) ---------------------------------
// (g, split) = the workgroup's group and row split (blockIdx.x, blockIdx.y of the standalone launch).  LDS (floats): smem [4 C C] | csl [4][C]
constexpr int APPLYWG64_LDS_FLOATS = 4 * 64 * 64 + 4 * 64;

template <int KIND, int CHAIN>
__device__ __forceinline__ void applywg64_body(const float* __restrict__ dOut, const float* __restrict__ Y, const float* __restrict__ S,
                                               const float* __restrict__ W, long w_gstride, const float* __restrict__ resid,
                                               const float* __restrict__ resid2, float* __restrict__ dS, float* __restrict__ dW,
                                               float* __restrict__ colsum, RowMap rm, int tiles_per_wave, int g, int split, float* __restrict__ lds) {
    constexpr int C = 64, TP = C + 4;
    float* smem = lds;                                                          // fold [4][C*C]; first: Wl [C*C] | 4 tiles [16][TP]
    float (*csl)[C] = reinterpret_cast<float (*)[C]>(lds + 4 * C * C);
    float* Wl = smem;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* tile = smem + C * C + wave * 16 * TP;
    const int j = lane & 15, kk = lane >> 4;
    const int ntiles = (rm.M + 15) / 16;
    const int t0 = (split * 4 + wave) * tiles_per_wave, t1 = min(ntiles, t0 + tiles_per_wave);
    float4 d[4], y[4], a[4];
    auto fetch = [&](int t) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int m = min(t * 16 + 4 * s4 + kk, rm.M - 1);
            const size_t off = ((size_t)g * rm.rs_g + (size_t)m * rm.rs_m) * C + 4 * j;
            d[s4] = ld4(dOut + off); a[s4] = ld4(S + off);
            if (KIND == 0 && CHAIN == 0) y[s4] = ld4(Y + off);
        }
    };
    if (t0 < t1) fetch(t0);                          // in flight while the weight is staged
    load_w_lds<C, 256>(Wl, W + (size_t)g * w_gstride, KIND == 0 ? 1 : 0, threadIdx.x);     // KIND 0: W_g^T (dS = dPre W_g^T); 1: Wp as stored
    __syncthreads();
    float4 bv[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[q][e] = ld4(Wl + (16 * q + 4 * kk + e) * C + 4 * j);
    f32x4 accw[4][4];
#pragma unroll
    for (int ca = 0; ca < 4; ++ca)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) accw[ca][cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float4 cs = f4zero();
    for (int t = t0; t < t1; ++t) {
        if (KIND == 1 && t != t0) fetch(t);          // (KIND 1 keeps no prefetch: its epilogue operands need the registers)
        SB();
        // ---- dPre in the weight-gradient layout; rows beyond M contribute nothing ----
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            float4 v = d[s4];
            if (KIND == 0 && CHAIN == 0) v = make_float4(d[s4].x * lrelu_grad_from_out(y[s4].x), d[s4].y * lrelu_grad_from_out(y[s4].y),
                                                         d[s4].z * lrelu_grad_from_out(y[s4].z), d[s4].w * lrelu_grad_from_out(y[s4].w));
            if (t * 16 + 4 * s4 + kk >= rm.M) v = f4zero();
            d[s4] = v;
            cs = f4add(cs, v);
            st4(tile + (4 * s4 + kk) * TP + 4 * j, v);
        }
        // ---- dW += S^T dPre: component ca of S / cb of dPre feed accumulator tile (ca, cb) (as wgrad64_kernel) ----
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            // KIND 0: dW = S^T dPre ([in][out]);  KIND 1: dWp = dY^T X ([out][in]) — the roles of the two operands swap
            const float sv[4] = {a[s4].x, a[s4].y, a[s4].z, a[s4].w}, dv[4] = {d[s4].x, d[s4].y, d[s4].z, d[s4].w};
#pragma unroll
            for (int ca = 0; ca < 4; ++ca)
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
                    accw[ca][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(KIND == 0 ? sv[ca] : dv[ca], KIND == 0 ? dv[cb] : sv[cb], accw[ca][cb], 0, 0, 0);
        }
        SB();
        // ---- dPre tile back in the data-gradient operand layout (wave-private tile: no barrier) ----
        float4 ap[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ap[q] = ld4(tile + j * TP + 16 * q + 4 * kk);
        const int tcur = t;
        if (KIND == 0 && t + 1 < t1) fetch(t + 1);   // next tile's operands: in flight during the 64 MFMAs below
        float4 rv[4], rv2[4];
        if (KIND == 1 || CHAIN == 2) {               // residual branch operands / sign operand of the epilogue, in the D layout
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = min(tcur * 16 + kk * 4 + r, rm.M - 1);
                const size_t off = ((size_t)g * rm.rs_g + (size_t)m * rm.rs_m) * C + 4 * j;
                if (KIND == 1) rv[r] = ld4(resid + off);
                if (KIND == 1 && CHAIN != 1) rv2[r] = ld4(resid2 + off);
                if (KIND == 0 && CHAIN == 2) rv2[r] = ld4(S + off);
            }
        }
        SB();
        f32x4 acc[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float av[4] = {ap[q].x, ap[q].y, ap[q].z, ap[q].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[q][e].x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[q][e].y, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[q][e].z, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[q][e].w, acc[3], 0, 0, 0);
            }
        }
        SB();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = tcur * 16 + kk * 4 + r;
            float4 o4 = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
            if (KIND == 1 && CHAIN == 0) {
                o4.x = fmaf(rv[r].x, lrelu_grad_from_out(rv2[r].x), o4.x); o4.y = fmaf(rv[r].y, lrelu_grad_from_out(rv2[r].y), o4.y);
                o4.z = fmaf(rv[r].z, lrelu_grad_from_out(rv2[r].z), o4.z); o4.w = fmaf(rv[r].w, lrelu_grad_from_out(rv2[r].w), o4.w);
            }
            if (KIND == 1 && CHAIN != 0) o4 = f4add(o4, rv[r]);
            if (CHAIN == 2) {
                o4.x *= lrelu_grad_from_out(rv2[r].x); o4.y *= lrelu_grad_from_out(rv2[r].y);
                o4.z *= lrelu_grad_from_out(rv2[r].z); o4.w *= lrelu_grad_from_out(rv2[r].w);
            }
            if (m < rm.M) st4(dS + ((size_t)g * rm.rs_g + (size_t)m * rm.rs_m) * C + 4 * j, o4);
        }
    }
    // ---- column sums of dPre (bias gradient partial of this row split) and the weight-gradient fold ----
    cs.x += __shfl_xor(cs.x, 16, 64); cs.y += __shfl_xor(cs.y, 16, 64); cs.z += __shfl_xor(cs.z, 16, 64); cs.w += __shfl_xor(cs.w, 16, 64);
    cs.x += __shfl_xor(cs.x, 32, 64); cs.y += __shfl_xor(cs.y, 32, 64); cs.z += __shfl_xor(cs.z, 32, 64); cs.w += __shfl_xor(cs.w, 32, 64);
    if (kk == 0) st4(&csl[wave][4 * j], cs);
    __syncthreads();                                 // every wave is done with Wl and its tile: smem becomes the fold buffer
    float* red = smem + wave * C * C;
#pragma unroll
    for (int ca = 0; ca < 4; ++ca)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            st4(&red[(4 * (kk * 4 + r) + ca) * C + 4 * j], make_float4(accw[ca][0][r], accw[ca][1][r], accw[ca][2][r], accw[ca][3][r]));
    __syncthreads();
    if (colsum != nullptr && threadIdx.x < C)
        colsum[((size_t)split * rm.G + g) * C + threadIdx.x] = (csl[0][threadIdx.x] + csl[1][threadIdx.x]) + (csl[2][threadIdx.x] + csl[3][threadIdx.x]);
    float* o = dW + ((size_t)split * rm.G + g) * (size_t)(C * C);
#pragma unroll
    for (int k = 0; k < C * C / 4 / 256; ++k) {
        const int f = threadIdx.x + k * 256;
        const float4 s4 = f4add(f4add(ld4(smem + 4 * f), ld4(smem + C * C + 4 * f)), f4add(ld4(smem + 2 * C * C + 4 * f), ld4(smem + 3 * C * C + 4 * f)));
        st4(o + 4 * f, s4);
    }
}

// ---- guide classifier: node layer + ln1 backward on the low-rank form (guidein.hip; see the comment at the top of that file) -------------
// n = the workgroup's node.  LDS (floats): red [RPP][2][C] | vec [2 C]
template <int C>
constexpr int guide_in_bwd_lds_floats() { return (256 / (C / 4)) * 2 * C + 2 * C; }

template <int C>
__device__ __forceinline__ void guide_in_bwd_body(const float* __restrict__ dPre, const float* __restrict__ src, int lda,
                                                  const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ Wn,
                                                  float* __restrict__ dWb, float* __restrict__ dinp, int BT, int N, int n, float* __restrict__ lds) {
    constexpr int LPR = C / 4, RPP = 256 / LPR, U = 6, PP = 256 / C;
    float* red = lds;
    float* vec = lds + RPP * 2 * C;
    const int tid = threadIdx.x;
    const int slot = tid / LPR, c4 = tid % LPR;
    float4 P = f4zero(), Q = f4zero();
    for (int rr = slot; rr < BT; rr += RPP * U) {             // U rows of loads in flight per thread (rows of node n: stride N*C floats)
        float4 d[U];
        float s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t r = (size_t)min(rr + u * RPP, BT - 1) * N + n;
            d[u] = ld4(dPre + r * C + 4 * c4);
            s[u] = src[r * lda];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (rr + u * RPP < BT) { P = f4fma(s[u], d[u], P); Q = f4add(Q, d[u]); }
    }
    st4(red + (slot * 2 + 0) * C + 4 * c4, P); st4(red + (slot * 2 + 1) * C + 4 * c4, Q);
    __syncthreads();
    for (int i = tid; i < 2 * C; i += 256) {                 // fold the slots in order
        float s = 0.f;
#pragma unroll 4
        for (int sl = 0; sl < RPP; ++sl) s += red[(sl * 2 + i / C) * C + i % C];
        vec[i] = s;
    }
    __syncthreads();
    float* row = dWb + (size_t)n * (C * C + C);
    for (int f = tid; f < C * C / 4; f += 256) {             // dW_n = w1^T (x) p + b1^T (x) q
        const int i = f / LPR, o4 = f % LPR;
        const float wi = w1[i], bb = b1[i];
        const float4 p4 = ld4(vec + 4 * o4), q4 = ld4(vec + C + 4 * o4);
        st4(row + (size_t)i * C + 4 * o4, make_float4(fmaf(wi, p4.x, bb * q4.x), fmaf(wi, p4.y, bb * q4.y), fmaf(wi, p4.z, bb * q4.z), fmaf(wi, p4.w, bb * q4.w)));
    }
    if (tid < C) row[C * C + tid] = vec[C + tid];            // db_n
    {   // [W_n p | W_n q]: thread (input channel i, part of the output channels)
        const int i = tid / PP, pq = tid % PP;
        const float* Wr = Wn + (size_t)n * C * C + (size_t)i * C + pq * (C / PP);
        float r1 = 0.f, r2 = 0.f;
#pragma unroll
        for (int k = 0; k < C / PP / 4; ++k) {
            const float4 x = ld4(Wr + 4 * k);
            r1 += f4dot(x, ld4(vec + pq * (C / PP) + 4 * k));
            r2 += f4dot(x, ld4(vec + C + pq * (C / PP) + 4 * k));
        }
        r1 = group_sum<PP>(r1); r2 = group_sum<PP>(r2);
        if (pq == 0) { dinp[(size_t)n * 2 * C + i] = r1; dinp[(size_t)n * 2 * C + C + i] = r2; }
    }
}

// ---- one guest of a host launch: the operands of one KL-path stage (gptst_hypertem_chain_fwd_kl) -------------------------------------------
struct KlGuest {
    int base;            // the host's own workgroups: guest workgroup v = blockIdx.x - base
    int v0;              // first virtual block of this launch's share of the stage (the time-conditioned layer may be split over two hosts)
    TailArgs tail;       // stage 1 (tail_mfma_body<1, 64>)
    // stage 2: applywg64_body<0, 2> (dOut = d_h2 as dPre, S = h1, W = W_bt), G = rm.G groups x row splits
    const float* dOut; const float* S; const float* W; float* dS; float* dW; float* colsum; RowMap rm; int tpw;
    // stage 3: guide_in_bwd_body<64>
    const float* dPre; const float* src; int lda; const float* w1; const float* b1; const float* Wn; float* dWb; float* dinp; int BT, N;
};

// STAGE 1..3: run virtual block v of that stage with the host's LDS (the caller has checked that v is one of the stage's blocks)
template <int STAGE>
__device__ __forceinline__ void kl_guest_run(const KlGuest& k, int v, float* lds) {
    if constexpr (STAGE == 1) tail_mfma_body<1, 64>(k.tail, v, lds);
    else if constexpr (STAGE == 2) applywg64_body<0, 2>(k.dOut, nullptr, k.S, k.W, 64L * 64, nullptr, nullptr, k.dS, k.dW, k.colsum, k.rm, k.tpw,
                                                        v % k.rm.G, v / k.rm.G, lds);
    else guide_in_bwd_body<64>(k.dPre, k.src, k.lda, k.w1, k.b1, k.Wn, k.dWb, k.dinp, k.BT, k.N, v, lds);
}

// LDS (bytes) a guest of STAGE needs from its host
inline size_t kl_guest_lds_bytes(int stage) {
    const int f = stage == 1 ? tail_mfma_lds_floats<64>() : stage == 2 ? APPLYWG64_LDS_FLOATS : guide_in_bwd_lds_floats<64>();
    return (size_t)f * sizeof(float);
}
