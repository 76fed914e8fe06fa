// Shared device helpers for the gfx950 (CDNA4, wave64) kernels of the GPT-ST pretraining path.
// Everything here is fp32: the reference computes in fp32 and parity is 1e-4 rel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gptst_hip.h"               // the exported prototypes: default visibility (the build is -fvisibility=hidden) and checked against
#include "gptst_hip_testing.h"       // the definitions by the compiler

#define GPTST_OK 0
#define GPTST_EARG (-1)      // bad argument (shape / null pointer)
#define GPTST_ESHAPE (-2)    // shape not supported by the compiled kernels
#define GPTST_EWS (-3)       // workspace too small

#define LRELU_SLOPE 0.01f

// cross-file helpers that are not part of the C ABI (include/gptst_hip.h): C linkage for the linker, hidden from the .so's exports
#define GPTST_INTERNAL extern "C" __attribute__((visibility("hidden")))
// In-kernel s_memtime stamps, phase-ablation flags and the entry points that drive them exist only in -DGPTST_DEBUG builds
// (GPTST_EXTRA_HIPCC_FLAGS=-DGPTST_DEBUG python -m gptst_amd.build --force): the product library carries none of them.

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define GPTST_CHECK_LAUNCH()                                  \
    do {                                                      \
        hipError_t e__ = hipGetLastError();                   \
        if (e__ != hipSuccess) return (int)e__;               \
    } while (0)

// ---- per-workgroup phase stamps (-DGPTST_STAMPS builds only: tools/phase_stamps.py) -----------------------------------------------------
// GPTST_STAMP(i) records the wall clock (100 MHz) of stamp i for a few chosen workgroups (wave 0, lane 0) and, as stamp 0 / 31, every
// workgroup's start / end goes to a second table — the schedule of a launch (who ran when, next to whom) is what located the prologue
// bursts of cap_route_fwd.  Each translation unit has its own tables and exports gptst_stamps_<unit>(out).
#ifdef GPTST_STAMPS
#define GPTST_STAMP_TABLES(unit)                                                                                       \
    __device__ long long g_st_ph[8][32];                                                                               \
    __device__ long long g_st_wg[2048][2];                                                                             \
    extern "C" __attribute__((visibility("default"))) int gptst_stamps_##unit(long long* ph, long long* wg) {          \
        if (ph && hipMemcpyFromSymbol(ph, HIP_SYMBOL(g_st_ph), sizeof(long long) * 8 * 32) != hipSuccess) return 1;   \
        if (wg && hipMemcpyFromSymbol(wg, HIP_SYMBOL(g_st_wg), sizeof(long long) * 2048 * 2) != hipSuccess) return 1; \
        return 0;                                                                                                      \
    }
// slots: workgroups 5, 100, 200, 300 (+ 261, 383 for second residents), first wave
#define GPTST_STAMP(i) do { if ((threadIdx.x & 63) == 0 && (threadIdx.x >> 6) == 0) { const int b_ = blockIdx.x;               \
        const int sl_ = b_ == 5 ? 0 : b_ == 100 ? 1 : b_ == 200 ? 2 : b_ == 300 ? 3 : b_ == 261 ? 4 : b_ == 383 ? 5 : -1;        \
        if (sl_ >= 0) g_st_ph[sl_][i] = wall_clock64(); } } while (0)
#define GPTST_WG_BEGIN() do { if (threadIdx.x == 0 && blockIdx.x < 2048) g_st_wg[blockIdx.x][0] = wall_clock64(); } while (0)
#define GPTST_WG_END() do { if (threadIdx.x == 0 && blockIdx.x < 2048) g_st_wg[blockIdx.x][1] = wall_clock64(); } while (0)
#else
#define GPTST_STAMP_TABLES(unit)
#define GPTST_STAMP(i) do { } while (0)
#define GPTST_WG_BEGIN() do { } while (0)
#define GPTST_WG_END() do { } while (0)
#endif

// Phase fence for the machine scheduler: instructions are not moved across it.  The kernels are written as explicit phases (batch
// of global loads -> LDS / MFMA -> prefetch of the next tile -> stores) and lose 10-40 % when the compiler re-interleaves them.
#ifdef GPTST_NO_SB
#define SB() do { } while (0)
#else
#define SB() __builtin_amdgcn_sched_barrier(0)
#endif

// Deterministic mode (gptst_set_deterministic): the few reductions that still end in float atomics (embedding gradients of the pool
// jobs, time-feature weight gradients) switch to single-owner kernels with a fixed summation order, so that two runs of a step are
// bit-identical.  Everything else is order-fixed by construction (partials + ordered folds, "last workgroup folds" for scalars).
extern thread_local int g_deterministic;

// "last workgroup folds": every workgroup publishes its partial with st_agent() (write-through stores, thread 0), takes a ticket, and
// the one that draws the last ticket sums all partials (ld_agent()) in index order — the result does not depend on which workgroup
// that is.  Returns true in the last workgroup (all threads).  No agent-scope FENCE: a release fence writes back every dirty L2 line of
// the XCD (the kernel's own 16.7 MB output) — 510 workgroups doing that cost ~20 us; write-through payload + drained vmcnt + relaxed
// agent-scope ticket is the cheap valid form (MI355X_MICROARCH.md, inter-workgroup visibility).
__device__ __forceinline__ void st_agent(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ld_agent(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// 16-byte forms over a buffer resource (rs: __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, 0x00020000) with a WAVE-UNIFORM base; off in
// bytes): sc1 = agent scope, i.e. the store is written through to memory and the load does not trust another XCD's stale L2 line.  A producer
// follows its stores with `s_waitcnt vmcnt(0)` + __syncthreads() and one relaxed agent-scope flag store (MI355X_MICROARCH.md, inter-workgroup
// visibility); the consumer polls the flag with ONE lane, relaxed, BOUNDED, then loads with ld4_sc1.
// Publish / consume fences of the hand-offs.  The protocol in use is the one MI355X_MICROARCH.md lists as valid without a fence pair: payload written
// THROUGH (sc1 stores), every storing wave drains vmcnt, a barrier, one relaxed agent-scope flag store; the consumer polls relaxed with one lane and
// reads the payload with sc1 loads ("sc1 loads may replace the acquire only when the producer stored sc1").  -DGPTST_HANDOFF_FENCES adds the
// release / acquire pair on top (buffer_wbl2 sc1 + s_waitcnt in the publishing lane, buffer_inv sc1 in the polling lane) — the form VERDICT r04
// asked for; its measured cost is in DESIGN.md section 10 (the release writes back every dirty L2 line of the XCD, i.e. the kernel's own output).
__device__ __forceinline__ void gptst_publish_fence() {
#ifdef GPTST_HANDOFF_FENCES
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
}
__device__ __forceinline__ void gptst_consume_fence() {
#ifdef GPTST_HANDOFF_FENCES
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
}
// Bounded wait of ONE lane for a hand-off word written by another workgroup of the same launch: relaxed agent-scope polls, s_sleep between
// them, and a WALL-CLOCK bound (2 s of the 100 MHz counter) — a spin COUNT is not a time: when another process shares the GPU its time
// slices stall the producer while the consumer's polls keep counting (4000 polls expired about once in four runs of the two-ranks-on-one-GPU
// test).  false = the hand-off is lost: the caller poisons its output with NaN, so the run ends loudly instead of hanging the GPU.
__device__ __forceinline__ bool gptst_wait_ge(const unsigned* p, unsigned want, unsigned* lost) {
    const long long t0 = wall_clock64();
    for (;;) {
#pragma unroll 1
        for (int i = 0; i < 64; ++i) {
            if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) { gptst_consume_fence(); return true; }
            __builtin_amdgcn_s_sleep(8);
        }
        if (wall_clock64() - t0 > 200000000LL) { atomicAdd(lost, 1u); return false; }      // 2 s
    }
}
// Every translation unit with such waits counts its expiries (a __device__ word; gptst_handoff_timeouts() adds them up for the host): a NaN loss
// can then be told from numerical trouble, and a run without NaN can still prove that no wait ever expired.
#define GPTST_HANDOFF_COUNTER(unit)                                                                  \
    __device__ unsigned g_handoff_lost_##unit = 0u;                                                  \
    GPTST_INTERNAL int gptst_handoff_lost_##unit(unsigned* out) {                                    \
        return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_handoff_lost_##unit), sizeof(unsigned)) == hipSuccess ? 0 : 1;   \
    }                                                                                                \
    GPTST_INTERNAL const unsigned* gptst_handoff_word_##unit(void) {      /* device address of the counter (the optimiser's guard reads it) */ \
        void* p_ = nullptr;                                                                          \
        return hipGetSymbolAddress(&p_, HIP_SYMBOL(g_handoff_lost_##unit)) == hipSuccess ? (const unsigned*)p_ : nullptr;   \
    }                                                                                                \
    GPTST_INTERNAL int gptst_handoff_clear_##unit(unsigned to) {                                     \
        const unsigned z_ = to;                                                                      \
        return hipMemcpyToSymbol(HIP_SYMBOL(g_handoff_lost_##unit), &z_, sizeof(unsigned)) == hipSuccess ? 0 : 1;   \
    }
typedef int gptst_i32x4 __attribute__((ext_vector_type(4)));
typedef float gptst_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st4_sc1(__amdgpu_buffer_rsrc_t rs, int off, float4 v) {
    const gptst_f32x4 f = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(gptst_i32x4, f), rs, off, 0, 16);
}
__device__ __forceinline__ float4 ld4_sc1(__amdgpu_buffer_rsrc_t rs, int off) {
    const gptst_f32x4 f = __builtin_bit_cast(gptst_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16));
    return make_float4(f[0], f[1], f[2], f[3]);
}
__device__ __forceinline__ bool last_block_arrives(unsigned* ticket, unsigned nblocks) {
    __shared__ unsigned s_last;
    if (threadIdx.x == 0) {                                          // thread 0 published the partials: drain its stores, then arrive
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_last = (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nblocks - 1) ? 1u : 0u;
    }
    __syncthreads();
    return s_last != 0u;
}

__device__ __forceinline__ float lrelu(float x) { return x > 0.f ? x : LRELU_SLOPE * x; }
// derivative selected by the sign of the OUTPUT (slope > 0 keeps the sign; x == 0 -> slope, as ATen).
__device__ __forceinline__ float lrelu_grad_from_out(float out) { return out > 0.f ? 1.f : LRELU_SLOPE; }

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// StandardScaler.inverse_transform (reference lib/normalization.py:23-27) as fp32 torch forms it: a rounded multiply, then a rounded add.
// The loss and the metrics keep a cell by `y > thresh` on this value, so the rounding is part of the rule: a stored raw zero
// fl32((0 - mu) / sigma) comes back as exactly 0.0 (or within an ulp of mu) here, and as a residual of either sign from one fused
// multiply-add — which `x * sigma + mu` compiles to under hipcc's default contraction.  (__fmul_rn / __fadd_rn are plain `*` / `+` in this
// toolchain's headers and would be fused after inlining all the same; the pragma takes the contract flag off the two operations.)
__device__ __forceinline__ float inverse_transform(float x, float sigma, float mu) {
#pragma clang fp contract(off)
    const float scaled = x * sigma;
    return scaled + mu;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// store of a tensor whose consumer is far away (the saved mix R of hyperTem: read by the backward ~0.5 ms later).  -DHT_R_NT: nontemporal.
__device__ __forceinline__ void st4_far(float* p, float4 v) {
#ifdef HT_R_NT
    typedef float gptst_v4f_ __attribute__((ext_vector_type(4)));
    const gptst_v4f_ t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<gptst_v4f_*>(p));
#else
    st4(p, v);
#endif
}
__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4fma(float s, float4 a, float4 c) {
    return make_float4(fmaf(s, a.x, c.x), fmaf(s, a.y, c.y), fmaf(s, a.z, c.z), fmaf(s, a.w, c.w));
}
__device__ __forceinline__ float f4dot(float4 a, float4 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); }

// ---- wave-level segmented reductions -------------------------------------------------------------------------------
// Groups of W consecutive lanes (W power of two <= 64); every lane of a group ends with the group's total.
// Up to 16 lanes (one DPP row) the exchange is done with DPP modifiers (VALU latency, no LDS crossbar):
// quad_perm[1,0,3,2] (0xB1), quad_perm[2,3,0,1] (0x4E), row_half_mirror (0x141), row_mirror (0x140); beyond a row
// it falls back to ds_bpermute (__shfl_xor).
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int W>
__device__ __forceinline__ float group_sum(float v) {
    if (W >= 2) v += dpp_mov<0xB1>(v);
    if (W >= 4) v += dpp_mov<0x4E>(v);
    if (W >= 8) v += dpp_mov<0x141>(v);
    if (W >= 16) v += dpp_mov<0x140>(v);
    if (W >= 32) v += __shfl_xor(v, 16, 64);
    if (W >= 64) v += __shfl_xor(v, 32, 64);
    return v;
}
template <int W>
__device__ __forceinline__ float group_max(float v) {
    if (W >= 2) v = fmaxf(v, dpp_mov<0xB1>(v));
    if (W >= 4) v = fmaxf(v, dpp_mov<0x4E>(v));
    if (W >= 8) v = fmaxf(v, dpp_mov<0x141>(v));
    if (W >= 16) v = fmaxf(v, dpp_mov<0x140>(v));
    if (W >= 32) v = fmaxf(v, __shfl_xor(v, 16, 64));
    if (W >= 64) v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}

// squash scale for a vector with squared norm sq:  y = x * sq / ((1+sq) * (sqrt(sq)+1e-8))   (reference GPTST.py:36-39)
__device__ __forceinline__ float squash_scale(float sq) { return (sq / (1.f + sq)) / (sqrtf(sq) + 1e-8f); }
