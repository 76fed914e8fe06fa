// The semantic view of the downstream DMVSTNET predictor (reference model/DMVSTNET_demand/DMVSTNET.py:57-61; gpt-st_amd/predictors/dmvstnet.py,
// dmvstnet_hip.py) — the one part of that model no earlier kernel serves.  There is no nonlinearity between the view and the model's 2-column
// output, so Lin_in_sen, the per-node (h, h) weight generated from the node embedding and the head's columns over the view compose to one
// per-node thin projection of x itself:  z[r, :] = x[r, :] V[n] + c[n],  n = r mod N, V (N, C, O), c (N, O) (formed by torch from the five
// parameters, a few hundred KB).  A workgroup owns 16 nodes and a contiguous range of the (b, t) units; a node's 16 lanes hold V[n] in
// registers, 4 channels a lane (8 at C > 64), and walk the units:
//   forward    z = the 16 lanes' partial dot products folded by four xor shuffles (a fixed order) + c
//   backward   dx = dz V[n]^T;  dV[n] and dc[n] accumulate over the workgroup's units in ascending order and leave as the split's partial
//              (nsplit, N, C, O), (nsplit, N, O); the caller sums the splits in order
// Memory-bound on one read of x; no LDS, no float atomics, no workgroup waits on another: two runs are bit-equal.
// (The temporal view's LSTM runs on csrc/stmgcn.hip's entries at one layer.  A variant of those kernels that applied the head's columns over h
// inside the launches was built and measured slower forward + backward than the plain entries with a torch head: DESIGN.md section 33.)
#include "common.h"
#include "gptst_hip.h"

#define DM_THREADS 256
#define DM_MAXSPLIT 64
#define DM_MAXO 4

// ---- the launch parameters ------------------------------------------------------------------------------------------------------------------
struct DmSen {
    int units, N, C, per;          // per: units a split owns
    const float* x;                // (units, N, C)
    const float* V;                // (N, C, O)
    const float* c;                // (N, O)
    float* z;                      // forward: (units, N, O)
    const float* dz;               // backward: (units, N, O)
    float *dx, *pV, *pc;           // (units, N, C);  (nsplit, N, C, O);  (nsplit, N, O)
};

// thread = (node n0 + tid / 16, lane16 = tid % 16): channels 4 lane16 .. + 3 of each 64-channel chunk
template <int O, bool BWD>
__global__ __launch_bounds__(DM_THREADS) void dm_sen_kernel(DmSen p) {
    const int tid = threadIdx.x, q = tid & 15, n = blockIdx.x * 16 + (tid >> 4);
    const int N = p.N, C = p.C;
    const bool node = n < N;                                               // (a node's 16 lanes agree: the shuffles below stay among them)
    const int u0 = blockIdx.y * p.per, u1 = min(u0 + p.per, p.units);
    float v[2][4][O], aV[2][4][O], ac[O];
    bool on[2];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        const int c0 = 64 * ch + 4 * q;
        on[ch] = node && c0 < C;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int o = 0; o < O; ++o) {
                v[ch][i][o] = on[ch] ? p.V[((size_t)n * C + c0 + i) * O + o] : 0.f;
                aV[ch][i][o] = 0.f;
            }
    }
    float cn[O];
#pragma unroll
    for (int o = 0; o < O; ++o) {
        cn[o] = (!BWD && node) ? p.c[(size_t)n * O + o] : 0.f;
        ac[o] = 0.f;
    }
    for (int u = u0; u < u1; ++u) {
        const size_t r = (size_t)u * N + (node ? n : 0);
        float4 xv[2];
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) xv[ch] = on[ch] ? ld4(p.x + r * C + 64 * ch + 4 * q) : f4zero();
        if constexpr (!BWD) {
            float s[O];
#pragma unroll
            for (int o = 0; o < O; ++o) {
                s[o] = 0.f;
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    s[o] = fmaf(xv[ch].x, v[ch][0][o], s[o]);
                    s[o] = fmaf(xv[ch].y, v[ch][1][o], s[o]);
                    s[o] = fmaf(xv[ch].z, v[ch][2][o], s[o]);
                    s[o] = fmaf(xv[ch].w, v[ch][3][o], s[o]);
                }
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) s[o] += __shfl_xor(s[o], m);
            }
            if (node && q == 0) {
#pragma unroll
                for (int o = 0; o < O; ++o) p.z[r * O + o] = s[o] + cn[o];
            }
        } else {
            float d[O];
#pragma unroll
            for (int o = 0; o < O; ++o) {
                d[o] = node ? p.dz[r * O + o] : 0.f;
                ac[o] += d[o];
            }
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const float xs[4] = {xv[ch].x, xv[ch].y, xv[ch].z, xv[ch].w};
                float g[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    g[i] = 0.f;
#pragma unroll
                    for (int o = 0; o < O; ++o) {
                        g[i] = fmaf(d[o], v[ch][i][o], g[i]);
                        aV[ch][i][o] = fmaf(xs[i], d[o], aV[ch][i][o]);
                    }
                }
                if (on[ch]) *reinterpret_cast<float4*>(p.dx + r * C + 64 * ch + 4 * q) = make_float4(g[0], g[1], g[2], g[3]);
            }
        }
    }
    if constexpr (BWD) {
        const size_t sn = (size_t)blockIdx.y * N + n;
#pragma unroll
        for (int ch = 0; ch < 2; ++ch)
            if (on[ch]) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int o = 0; o < O; ++o) p.pV[(sn * C + 64 * ch + 4 * q + i) * O + o] = aV[ch][i][o];
            }
        if (node && q == 0) {
#pragma unroll
            for (int o = 0; o < O; ++o) p.pc[sn * O + o] = ac[o];
        }
    }
}

// units a split owns: splits until the grid has about four workgroups a CU, DM_MAXSPLIT at the most, none of them empty
static int dm_sen_per(int units, int N) {
    const int tiles = (N + 15) / 16;
    int ns = (1024 + tiles - 1) / tiles;
    if (ns > DM_MAXSPLIT) ns = DM_MAXSPLIT;
    if (ns > units) ns = units;
    return (units + ns - 1) / ns;
}

static int dm_sen_check(int units, int N, int C, int O) {
    if (units <= 0 || N <= 0) return GPTST_EARG;
    if (C < 16 || C > 128 || C % 16 || O < 1 || O > DM_MAXO || (long)units * N > 0x7fffffffL / 128 || (N + 15) / 16 > 65535) return GPTST_ESHAPE;
    return GPTST_OK;
}

extern "C" int gptst_dmvst_sen_nsplit(int units, int N) {
    if (units <= 0 || N <= 0) return GPTST_EARG;
    const int per = dm_sen_per(units, N);
    return (units + per - 1) / per;
}

template <bool BWD>
static int dm_sen_launch(const DmSen& p, int O, hipStream_t stream) {
    const dim3 grid((unsigned)((p.N + 15) / 16), (unsigned)((p.units + p.per - 1) / p.per));
    switch (O) {
    case 1: hipLaunchKernelGGL((dm_sen_kernel<1, BWD>), grid, dim3(DM_THREADS), 0, stream, p); break;
    case 2: hipLaunchKernelGGL((dm_sen_kernel<2, BWD>), grid, dim3(DM_THREADS), 0, stream, p); break;
    case 3: hipLaunchKernelGGL((dm_sen_kernel<3, BWD>), grid, dim3(DM_THREADS), 0, stream, p); break;
    default: hipLaunchKernelGGL((dm_sen_kernel<4, BWD>), grid, dim3(DM_THREADS), 0, stream, p); break;
    }
    GPTST_CHECK_LAUNCH();
    return GPTST_OK;
}

extern "C" int gptst_dmvst_sen_fwd(const float* x, const float* V, const float* c, float* z, int units, int N, int C, int O, void* stream) {
    if (!x || !V || !c || !z) return GPTST_EARG;
    const int rc = dm_sen_check(units, N, C, O);
    if (rc != GPTST_OK) return rc;
    DmSen p{};
    p.units = units; p.N = N; p.C = C; p.per = dm_sen_per(units, N); p.x = x; p.V = V; p.c = c; p.z = z;
    return dm_sen_launch<false>(p, O, (hipStream_t)stream);
}

extern "C" int gptst_dmvst_sen_bwd(const float* x, const float* V, const float* dz, float* dx, float* pV, float* pc, int nsplit, int units, int N,
                                   int C, int O, void* stream) {
    if (!x || !V || !dz || !dx || !pV || !pc) return GPTST_EARG;
    const int rc = dm_sen_check(units, N, C, O);
    if (rc != GPTST_OK) return rc;
    if (nsplit != gptst_dmvst_sen_nsplit(units, N)) return GPTST_EARG;
    DmSen p{};
    p.units = units; p.N = N; p.C = C; p.per = dm_sen_per(units, N); p.x = x; p.V = V; p.dz = dz; p.dx = dx; p.pV = pV; p.pc = pc;
    return dm_sen_launch<true>(p, O, (hipStream_t)stream);
}
