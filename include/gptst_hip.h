/* gptst_hip.h — C ABI of the MI355X (gfx950) GPT-ST pretraining kernels.
 *
 * Drop-in boundary: the reference has no FFI — its hot path sits behind the Python nn.Module
 * GPTST_Model (model/Pretrain_model/GPTST.py:459-493).  gpt-st_amd/model.py mirrors that interface and
 * calls these entry points through ctypes; each entry replaces the chain of ATen ops cited with it.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer into caller-owned memory (a torch tensor) that stays valid until
 *     the stream has executed the call; fp32 unless the name says otherwise; tensors are dense row-major;
 *   - activations are (B, T, N, C) = (B*T*N rows, C); T is 12 (reference GPTST.py:97,208-209);
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); calls only enqueue — no
 *     allocation, no synchronisation, no host reads — so a whole step can be captured in a hipGraph;
 *   - return 0 on success, a negative GPTST_E* code for bad arguments / unsupported shapes, or a positive
 *     hipError_t from the launch.  Never throws, never exits.
 *   - "+=" in a description means the kernel ACCUMULATES into the output (caller zeroes it once per step).
 */
#ifndef GPTST_HIP_H
#define GPTST_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: only what is declared between this push and the pop below is exported. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define GPTST_ABI_VERSION 30  /* 30: + gptst_dmvst_sen_* (the downstream DMVSTNET predictor on HIP: its semantic view as a per-node thin projection of x, forward and backward: csrc/dmvstnet.hip); 29: + gptst_ccrnn_* (the graph-GRU cell of the downstream CCRNN predictor on HIP: TGCN's GRU step with a multi-polynomial mix, the cell's input in the operand slab, the decoder's feedback formed while the slab is filled: csrc/ccrnn.hip); 28: + gptst_stmgcn_* (the stacked LSTM of the downstream ST-MGCN predictor on HIP: all T steps of all L layers in ONE launch forward and ONE backward, states in LDS, rows local to their workgroup: csrc/stmgcn.hip); 27: + gptst_stwa_* (the downstream ST-WA predictor on HIP: one cut of a Layer in two launches forward and three backward, generated per-node weights folded from their rank-5 factors, the spatial attention over the nodes of a sample without its N x N scores: csrc/stwa.hip); 26: + gptst_msdr_* (the multi-state recurrence of the downstream MSDR predictor on HIP: one launch per cell step forward, two backward, the attention logits from per-workgroup partials folded in a fixed order: csrc/msdr.hip); 25: + gptst_stgode_* (the downstream STGODE predictor on HIP: the fused Euler step forward and backward, its weight gradient and dW2 / dalpha reductions, batch norm over the node channel with the running max over the branches: csrc/stgode.hip); 24: + gptst_encin_ht1_bwd_jobs, gptst_gram_bwd_jobs, gptst_timefeat_jobs_bwd_jobs (the three launches at the end of the backward carry the gradient-reduction jobs as further workgroups: csrc/poolgen_dev.h pj_reduce_block); 23: + gptst_stfgnn_mix (the downstream STFGNN predictor on HIP: the product with the 4N x 4N spatial-temporal fusion graph as three N x N products per window: csrc/stfgnn.hip); gptst_stsgcn_wingemm / gptst_stsgcn_gate_bwd admit groups of R = 4N rows; 22: + gptst_stsgcn_* (the downstream STSGCN predictor on HIP: the localized window mix without its 3N x 3N matrix, a GEMM grouped by window with the running max, its gate backward and per-window weight gradient: csrc/stsgcn.hip); 21: + gptst_astgcn_* (the downstream ASTGCN predictor on HIP: node mixing with a per-sample masked graph, the gradient with respect to that graph, LayerNorm over the channels of a row: csrc/astgcn.hip); 20: + gptst_mtgnn_* (the downstream MTGNN predictor on HIP: tap GEMM between frames of different length, its weight gradient, the gate's backward, the gradient of the node mix with respect to its graphs: csrc/mtgnn.hip); 19: + gptst_tgcn_* (the recurrence of the downstream TGCN predictor on HIP, forward and backward: csrc/tgcn.hip); 18: + gptst_stgcn_* (the downstream STGCN predictor on HIP, forward and backward: csrc/stgcn.hip); 17: + gptst_fusion_gate_bwd_df (the gate's backward with the gradient of the embedding: fine-tuning the encoder downstream), gptst_deterministic_state; 16: + gptst_hypertem_chain_fwd_kl, gptst_kl_guest_blocks (the KL path's backward as guest workgroups of the forward's hyperTem chains); 15 (r06): + gptst_cap_split_units, gptst_cap_cross_route_lin_bwd_split (the last (b,t) units of the routing backward as two node halves: 384 units on 256 CUs -> one whole unit + one half per CU; measured, opt-in), gptst_clip_adam: stats_out[6] = updates skipped since gptst_handoff_reset; + gptst_mask_cooperative_state (the switch is thread-local now); + gptst_guide_head_fwd, gptst_guide_uc_floats (the guide classifier's forward in two launches); 14 (r05, late): + gptst_cap_cross_route_lin_bwd_jobs (gradient-reduction jobs as a role of the routing backward); 13 (r05, late): + gptst_mask_u24_fwd_jobs (forward generation jobs inside the cooperative mask launch); 12 (r05, late): + gptst_mask_cooperative (gptst_mask_*_u24 with 8192 < M <= 65536 cells and a workspace: ONE cooperative launch); 11 (r05): + gptst_cap_cross_route_lin_bwd, gptst_comm_available, gptst_handoff_reset, gptst_set_handoff_guard (gptst_clip_adam: stats_out[5] = expiries on record); - gptst_cap_rec_cross_route_bwd (three-role form, measured slower); 9, 10 (r04, late): + gptst_hypertem_bwd_pair, gptst_cap_rec_cross_route_bwd, gptst_mask_*_u24, gptst_pool_jobs_gram_rows, gptst_handoff_timeouts; gptst_fusion_gate_fwd/bwd */
int gptst_abi_version(void);
/* 1: bit-reproducible steps — the two reductions that end in float atomics by default (embedding gradients of gptst_pool_jobs kind 2,
 * weight gradients of gptst_timefeat_jobs) run as single-owner kernels with a fixed summation order (slower).  Everything else is
 * order-fixed by construction.  Thread-local. */
int gptst_set_deterministic(int on);
int gptst_deterministic_state(void);   /* the calling thread's setting (a caller that switches the mode for a few launches puts it back) */
/* Number of bounded in-launch hand-off waits that expired since the library was loaded (the roles of gptst_cap_cross_route_bwd /
 * gptst_cap_cross_route_lin_bwd, the lower weight-gradient role of gptst_hypertem_bwd_pair, the grid barriers of the cooperative mask launch
 * (gptst_mask_*_u24): a consumer workgroup waits at most 2 s of wall clock for its producer and poisons its output with NaN on expiry).  0 in a healthy run; lets a NaN loss be told from numerical trouble.  Synchronises. */
int gptst_handoff_timeouts(int* out);
/* r05: while an expiry is on record gptst_clip_adam SKIPS its update (weights and moments untouched; the count goes out in stats_out[5], and — r06 —
 * the number of updates skipped since the last gptst_handoff_reset() in stats_out[6]: a caller that enqueued several steps before it looked knows how many to take back) — the
 * caller re-runs the step without in-launch hand-offs and then clears the record with gptst_handoff_reset() (synchronises).
 * gptst_set_handoff_guard(0) turns the skip off (process-wide). */
int gptst_handoff_reset(void);
/* r05: gptst_mask_random_u24 / gptst_mask_adaptive_u24 with a workspace and 8192 < M <= 1048576 cells run as ONE launch of at most 128 workgroups of
 * 1024 threads (one cell per thread up to 131072 cells, two / four / eight beyond — r06: the global batch of up to eight bench-shape data-parallel ranks; digit histograms in the workspace, grid barriers with the bounded wait above; every workgroup is resident: at most
 * 128 on 256 CUs; the launcher takes this form only while the grid is at most HALF of what the device holds).  0: the multi-launch radix select instead (what a stepper falls back to after a lost hand-off); 1: on; < 0: the build's default
 * (on).  Thread-local (r06), like the other launch-mode switches.  Same masks bit for bit either way.  gptst_mask_cooperative_state(): the calling thread's setting (0 / 1) —
 * a scope that switches the form off restores what it found. */
int gptst_mask_cooperative(int on);
int gptst_mask_cooperative_state(void);
int gptst_set_handoff_guard(int on);

/* ---- embedding-conditioned parameter generation (poolgen.hip) -----------------------------------------
 * out[r,:] = sum_k emb[r,k] * pool[k,:]   r < R, k < K <= 16.  Optional second problem (pool2/out2/cols2) shares emb.
 * Replaces einsum('btd,dio->btio'), einsum('nd,dio->nio'), matmul(emb, bias_pool) (GPTST.py:24-25,29-30,137-138,
 * 160-161), einsum('btd,dhn->bthn') (:104), einsum('bd,dhk->bhk') (:129), einsum('nk,kht->nht') (:156). */
int gptst_poolgen_fwd(const float* emb, const float* pool, float* out, int cols, const float* pool2, float* out2,
                      int cols2, int R, int K, void* stream);
/* dpool[k,:] += sum_rr emb[rr % R, k] * dW[rr,:],  rr < R*nsplit (problem 1) / R (problem 2). */
int gptst_poolgen_bwd_pool(const float* emb, const float* dW, float* dpool, int cols, const float* dW2, float* dpool2,
                           int cols2, int R, int nsplit, int K, void* stream);
/* demb[r,k] += sum_s sum_c dW[s*R + r, c] pool[k,c]  (+ problem 2 without splits). */
int gptst_poolgen_bwd_emb(const float* dW, const float* pool, int cols, const float* dW2, const float* pool2, int cols2,
                          float* demb, int R, int nsplit, int K, void* stream);

/* multi-problem forms (<= 112 problems sharing emb; host arrays of device pointers, read at call time): one launch generates /
 * reduces the generated parameters of several layers (every launch has a ~4-5 us floor on MI355X). */
int gptst_poolgen_fwd_multi(const float* emb, int nprob, const void* pools, const void* outs, const int* cols, int R, int K,
                            void* stream);
int gptst_poolgen_bwd_pool_multi(const float* emb, int nprob, const void* dWs, const void* dpools, const int* cols, const int* nsplit,
                                 int R, int K, void* stream);
int gptst_poolgen_bwd_emb_multi(int nprob, const void* dWs, const void* pools, const int* cols, const int* nsplit, float* demb, int R,
                                int K, void* stream);

/* Job table: njobs independent problems of ANY kind, each with its own embedding and shapes, in ceil(njobs / 112) launches
 * (host arrays, read at call time).  kind 0: out (R,cols) = emb (R,K) . pool (K,cols);  kind 1: out = dpool (K,cols) += sum_rr
 * emb[rr % R,:]^T x[rr,:], rr < R*nsplit — owned by ONE workgroup per element (no atomics: two kind-1 jobs of one call must
 * not share `out`);  kind 2: out = demb (R,K) += (sum_s x[s*R + r,:]) . pool^T (atomic: several jobs may add into one demb).
 * kind 3: out (R,12,12) = A_r^T A_r with A_r = (emb . pool)[r] viewed as (cols/12, 12): hyperTem's per-node temporal graph (what
 * gptst_gram_fwd computes from a materialised A; bit-identical to it) without a launch of its own.
 * ldx[j]: row stride of x in floats (0 = cols) — a job may read a column window of a wider matrix.
 * Unused pointers of a kind may be NULL.  A whole pretraining step needs 3 calls (forward generation, two backward reductions)
 * where per-embedding launches needed ~50. */
int gptst_pool_jobs(int njobs, const int* kind, const void* const* emb, const void* const* x, const void* const* pool,
                    const void* const* out, const int* R, const int* K, const int* cols, const int* nsplit, const int* ldx, void* stream);
/* rows per workgroup of a kind-3 (temporal graph) job for (K, cols); <= 0: the shape does not fit the job kernel — use gptst_gram_fwd on the
 * forward job's output (more than 20 hyperedges at embed_dim 16). */
int gptst_pool_jobs_gram_rows(int K, int cols);

/* ---- C x C contractions on fp32 MFMA (apply.hip) ------------------------------------------------------
 * out[g,m,:] = epi( pro(A)[g,m,:] @ W[g] (+bias[g]) (+resid) ).   mode: 0 TIME (g=(b,t), rows n), 1 NODE (g=n, rows
 * (b,t)), 2 SHARED (one weight).  w_per_group: W is (G,C,C) else (C,C).  transw: W[g] stored [out][in].
 * pro: 0 none, 1 A*lrelu'(A2) (A=dOut, A2=layer output).  epi: 0 plain, 1 lrelu(acc+bias+resid),
 * 2 acc + resid*lrelu'(resid2) (adds the residual branch of a layer's backward), 3 lrelu(acc+bias),
 * 4 (C = 128, r05) (acc + resid)*lrelu'(resid2): the dPre-chain form of 2 (resid already is dPre, resid2 = the layer's INPUT);  5 (C = 128)
 * acc*lrelu'(resid2): the same without a residual branch.
 * colsum (optional): row-split PARTIALS of the bias gradient, colsum[s][g][:] = sum over the rows m of split s of pro(A)[g,m,:],
 *   s < gptst_apply_nsplit(mode, BT, N, C); plain stores in a fixed order (no atomics): the consumer sums the splits.
 * Replaces einsum('btni,btio->btno') / einsum('btni,nio->btno') + bias + residual + LeakyReLU
 * (GPTST.py:26-27,31-32,139-141,162-163), nn.Linear C->C (:102) and their backward w.r.t. the data. */
int gptst_apply_nsplit(int mode, int BT, int N, int C);
int gptst_apply(const float* A, const float* A2, const float* W, int w_per_group, int transw, const float* bias,
                const float* resid, const float* resid2, float* out, float* colsum, int mode, int pro, int epi, int BT,
                int N, int C, void* stream);
/* dW[s*G + g] = sum_{m in split s} A[g,m,:]^T pro(D)[g,m,:];  nsplit = gptst_wgrad_nsplit(mode,BT,N,C) partial sums
 * that the consumer (gptst_poolgen_bwd_*) adds up.  dW must hold nsplit*G*C*C floats. */
int gptst_wgrad_nsplit(int mode, int BT, int N, int C);
int gptst_wgrad(const float* A, const float* D, const float* D2, float* dW, int mode, int pro, int BT, int N, int C,
                void* stream);
/* same, with column sums appended to every split (rows of C*C + C floats): which = 1: [dW | sum_m A[m,:]] (weight AND bias gradient
 * of a shared Linear whose output gradient is A); which = 2: [dW | sum_m pro(D)[m,:]] (weight and bias gradient of a generated
 * layer, e.g. hyperTem's W_bt / b_bt — replaces a separate, atomically accumulated bias-gradient pass).  C = 64 or 128. */
int gptst_wgrad_colsum(const float* A, const float* D, const float* D2, float* dW, int mode, int pro, int which, int BT, int N, int C,
                       void* stream);

/* Backward of one generated-weight layer out = lrelu(S W_g + b_g [+ x]) in ONE pass (C = 64; mode 0 TIME / 1 NODE):
 * dPre = dOut*lrelu'(Y); dS = dPre W_g^T; per row split s < gptst_apply_wgrad_nsplit: dW[s][g] = S^T dPre, colsum[s][g] = column sums
 * of dPre (may be NULL).  Replaces gptst_apply(pro=1, transw=1, colsum) + gptst_wgrad(pro=1), which both read dOut and Y.
 * W (G,C,C) as in the forward ([in][out]).  Backward of einsum('btni,nio->btno') / ('btni,btio->btno') + bias + LeakyReLU
 * (GPTST.py:26-27,31-32,139-141).  dPre chain (see gptst_hypertem_bwd): Y == NULL -> dOut already is dPre; premul != 0 -> dS is
 * multiplied by lrelu'(S) (S = output of the LeakyReLU layer below). */
int gptst_apply_wgrad_nsplit(int mode, int BT, int N);
int gptst_apply_wgrad(const float* dOut, const float* Y, const float* S, const float* W, float* dS, float* dW, float* colsum, int premul,
                      int mode, int BT, int N, int C, void* stream);

/* Backward through the shared Linear at the entry of cap (P = squash(X Wp^T + bp), GPTST.py:102) plus the residual branch of the layer
 * (:139-141) in ONE pass: dX = dY Wp + dOut*lrelu'(out); per row split s < gptst_linear_bwd_nsplit(rows): dWp[s] = dY^T X ([out][in]),
 * dbp[s] = colsum(dY).  Replaces gptst_apply(mode 2, epi 2) + gptst_wgrad_colsum(mode 2).  C = 64.
 * dPre chain: out == NULL -> dOut already is dPre: dX = dY Wp + dPre, and with premul != 0  dX = (dY Wp + dPre) * lrelu'(X). */
int gptst_linear_bwd_nsplit(int rows);
int gptst_linear_bwd(const float* dY, const float* X, const float* Wp, const float* dOut, const float* out, float* dX, float* dWp, float* dbp,
                     int premul, int rows, int C, void* stream);

/* ---- per-node temporal hypergraph of hyperTem (tmix.hip), GPTST.py:156-158 -----------------------------
 * A (N,Hm,T) = node_emb . adj (via poolgen);  G[n] = A[n]^T A[n] (T x T);  ret[b,:,n,:] = G[n] X[b,:,n,:]. */
int gptst_gram_fwd(const float* A, float* G, int N, int Hm, void* stream);
/* gram_bwd: A (L*N,Hm,T) of L layers, dG (L, nsplit, N, T, T) PARTIAL graph gradients (e.g. one per sample from gptst_hypertem_bwd),
 * summed in a fixed order -> dA (L*N,Hm,T). */
int gptst_gram_bwd(const float* A, const float* dG, float* dA, int L, int N, int Hm, int nsplit, void* stream);
/* TAIL ROLES.  The end of a step's backward is off the data-gradient chain: gptst_encin_ht1_bwd, gptst_gram_bwd and the time-feature backward each run a
 * small latency-bound grid, and the gradient-reduction launch (gptst_pool_jobs kinds 1 / 2) is bandwidth work that needs no particular CU.  The three
 * *_jobs entries are the plain entry followed by gptst_pool_jobs(njobs, j...) in ONE launch: the grid is [the entry's workgroups | job blocks], the jobs
 * heaviest first; no workgroup waits for another.  The caller guarantees that the jobs' inputs were written by EARLIER launches of the stream, and that
 * the entry neither reads the jobs' outputs nor writes their inputs.  Every table is served: of more than 112 jobs the heaviest 112 ride and the
 * rest follow through gptst_pool_jobs; an empty table, the deterministic mode and a table with another kind give exactly the two calls.  Same
 * results as the two calls (kind-2 outputs are float atomics as in gptst_pool_jobs). */
int gptst_gram_bwd_jobs(const float* A, const float* dG, float* dA, int L, int N, int Hm, int nsplit,
                        int njobs, const int* jkind, const void* const* jemb, const void* const* jx, const void* const* jpool,
                        const void* const* jout, const int* jR, const int* jK, const int* jcols, const int* jnsplit, const int* jldx,
                        void* stream);
/* out = G (*) X  [+ dOut*lrelu'(Y) when dOut != NULL: fuses the residual branch of hyperTem's backward]. */
int gptst_tmix(const float* X, const float* G, const float* dOut, const float* Y, float* out, int B, int T, int N, int C,
               void* stream);
/* dG[n,t,u] = sum_{b,c} dR[b,t,n,c] X[b,u,n,c]   (fp32 MFMA 16x16x4). */
int gptst_tmix_dgraph(const float* dR, const float* X, float* dG, int B, int T, int N, int C, void* stream);
/* both of the above in one pass over dR (the unfused hyperTem backward, C = 128): dX = dOut*lrelu'(Y) + G (*) dR, dG = sum_b dR X^T */
int gptst_tmix_bwd(const float* dR, const float* X, const float* G, const float* dOut, const float* Y, float* dX, float* dG, int B, int T,
                   int N, int C, void* stream);
/* r05, the dPre-chain form of gptst_tmix_bwd (C = 128 path): dPre is the layer's pre-activation gradient (its output is not read);
 * dX = (dPre + G (*) dR), times lrelu'(X) when premul;  dG as above. */
int gptst_tmix_bwd_chain(const float* dR, const float* X, const float* G, const float* dPre, int premul, float* dX, float* dG, int B, int T,
                         int N, int C, void* stream);

/* fused hyperTem forward (hypertem.hip): R = G (*) X, out = LReLU(R W_bt + b_bt + X); one workgroup per (sample, 16 nodes), MFMA 16x16x4
 * with W_bt read from L2.  R_out: R kept for the weight gradient, or NULL (the backward then rebuilds it from X).  C = 64.
 * Replaces GPTST.py:157-158 + :162-163. */
int gptst_hypertem_fwd(const float* X, const float* G, const float* Wbt, const float* bbt, float* R_out, float* out, int B, int T,
                       int N, int C, void* stream);
/* hyperTem forward CHAIN (r04): nstage (1..3) consecutive hyperTem layers in ONE launch on the (sample, 16-node) slab — every one of them is
 * node-local, so a layer's output goes from the accumulators back into the LDS slab (and to HBM once, for the backward) and the next layer
 * starts from it: no load phase, no launch boundary in between.  X: the first layer's input.  Gs, Wbts, bbts, Rs, outs: HOST arrays of nstage
 * device pointers (G (N,T,T), W_bt (B*T,C,C), b_bt (B*T,C), R_out or NULL, out), read at call time.  Bit-identical to the per-layer calls.
 * C = 64 (GPTST_ESHAPE otherwise).  Replaces nstage x (GPTST.py:157-163) per launch.  (r05: the optional node-conditioned first stage of r04 —
 * measured slower than gptst_apply — left the signature.) */
int gptst_hypertem_chain_fwd(const float* X, int nstage, const void* Gs, const void* Wbts, const void* bbts, const void* Rs, const void* outs,
                             int B, int T, int N, int C, void* stream);
/* The same two-layer chain (nstage = 2) carrying virtual blocks [v0, v1) of one stage of the KL term's backward (BasicTrainer.py:85 through
 * MLP_RL, GPTST.py:21-33) as guest workgroups behind its own grid: the chain is one round of workgroups that leaves slots idle, and the KL path's
 * inputs exist once the encoder's first cap has routed.  Each guest block runs the body of the stand-alone kernel (bit-identical results):
 *   stage 1  gptst_tail_kl (premul = 1)                        ops = [h2, W3, prob, c, d_h2, part, sws], HS classes, weight w
 *   stage 2  gptst_apply_wgrad (MODE_TIME, Y = NULL, premul)   ops = [d_h2, h1, W_bt, d_h1, dW, db]
 *   stage 3  gptst_guide_in_bwd                                ops = [dPre, src, w1, b1, Wn, dWb, dinp], src rows of lda floats
 * ops: HOST array of device pointers, read at call time.  v1 <= gptst_kl_guest_blocks(stage, B, T, N); a stage may be split over several
 * launches.  C = 64, HS <= 16 (GPTST_ESHAPE otherwise). */
int gptst_hypertem_chain_fwd_kl(const float* X, int nstage, const void* Gs, const void* Wbts, const void* bbts, const void* Rs, const void* outs,
                                int B, int T, int N, int C, int stage, const void* ops, int v0, int v1, int HS, int lda, float w, void* stream);
/* number of virtual blocks of stage 1..3 of the KL path at this shape (the workgroups of its stand-alone launch) */
int gptst_kl_guest_blocks(int stage, int B, int T, int N);

/* Encoder input projection + the encoder's first hyperTem layer on the low-rank structure of the input (encin.hip, r04).  For base = 1 the
 * first activation is x0 = m w + bi (m = mask ? flow : fill, a scalar per row), so hyperTem1 needs neither x0 nor a GEMM:
 * out = LReLU(alpha (w W_bt) + beta (bi W_bt) + b_bt + m w + bi) with alpha = sum_u G_n[t,u] m_u, beta = sum_u G_n[t,u]; the backward collapses
 * the same way (rank-2 weight gradient, graph gradient from two dot products per row, input-projection gradient from per-(b,t) vectors).
 * fwd: src rows (B*T*N, lda) with the flow in column 0, mask (B*T*N) 1 = visible or NULL, w = dim_in_flow.weight (C,1), bi = its bias ->
 *      out (B,T,N,C), ab (B*T*N, 2) = (alpha, beta), wv (B*T, 2C) = (w W_bt | bi W_bt), both kept for the backward.
 * bwd: dPre = dOut * lrelu'(out) (chain form) -> dWb (B*T, C*C + C) rows [dW_bt | db_bt], dG (B,N,T,T) per-sample partials,
 *      dinp (B*T, 2C) partials of [d weight | d bias] of dim_in_flow (rows summed by the caller).
 * Replaces GPTST.py:418 + :154-163 of encoder.STHCN_encode.hyperTem1 and their backward.  base = 1, T = 12, C in {64, 128}; else GPTST_ESHAPE. */
int gptst_encin_ht1_fwd(const float* src, int lda, const float* mask, float fill, const float* w, const float* bi, const float* G,
                        const float* Wbt, const float* bbt, float* out, float* ab, float* wv, int B, int T, int N, int C, void* stream);
int gptst_encin_ht1_bwd(const float* dPre, const float* src, int lda, const float* mask, float fill, const float* w, const float* bi,
                        const float* Wbt, const float* ab, const float* wv, float* dWb, float* dG, float* dinp, int B, int T, int N, int C,
                        void* stream);
/* ... carrying a table of gradient-reduction jobs (TAIL ROLES, at gptst_gram_bwd_jobs); C = 128: the two calls */
int gptst_encin_ht1_bwd_jobs(const float* dPre, const float* src, int lda, const float* mask, float fill, const float* w, const float* bi,
                             const float* Wbt, const float* ab, const float* wv, float* dWb, float* dG, float* dinp, int B, int T, int N, int C,
                             int njobs, const int* jkind, const void* const* jemb, const void* const* jx, const void* const* jpool,
                             const void* const* jout, const int* jR, const int* jK, const int* jcols, const int* jnsplit, const int* jldx,
                             void* stream);

/* Guide classifier MLP_RL, input projection + node-conditioned layer on the low-rank structure of the input (guidein.hip, r04): for base = 1
 * h1 = LReLU((s w1 + b1) W_n + b_n) = LReLU(s u_n + c_n) with u_n = w1 W_n, c_n = b1 W_n + b_n — an elementwise pass; the backward needs
 * p_n = sum_rows s dPre and q_n = sum_rows dPre only: dW_n = w1^T (x) p_n + b1^T (x) q_n, db_n = q_n, d w1 = sum_n W_n p_n, d b1 = sum_n W_n q_n.
 * fwd: src rows (BT*N, lda) with the flow in column 0 -> h1 (BT*N, C).   bwd: dPre = dOut * lrelu'(h1) -> dWb (N, C*C + C) rows [dW_n | db_n],
 * dinp (N, 2C) partials of [d ln1.weight | d ln1.bias].  Replaces GPTST.py:22-27 and its backward.  base = 1, C in {64, 128}. */
int gptst_guide_in_fwd(const float* src, int lda, const float* w1, const float* b1, const float* Wn, const float* bn, float* h1, int BT, int N,
                       int C, void* stream);
int gptst_guide_in_bwd(const float* dPre, const float* src, int lda, const float* w1, const float* b1, const float* Wn, float* dWb, float* dinp,
                       int BT, int N, int C, void* stream);
/* r06: the classifier's whole forward (GPTST.py:21-34 + the softmax of :332 / :343 and the arg-max of :344-345) in two launches: the node vectors
 * u_n, c_n (N workgroups), then ONE pass grouped by (b,t): h1 = LReLU(s u_n + c_n) built in registers, h2 = LReLU(h1 W_bt + b_bt), logits = h2 W3^T + b3,
 * softmax, first-maximum label.  Replaces gptst_guide_in_fwd + gptst_apply(mode TIME, LReLU) + gptst_rowdot(softmax, label): same arithmetic in the
 * same order (bit-identical h1, h2, prob, label), three activation-sized round trips less.  uc: gptst_guide_uc_floats(N, C) floats of scratch.
 * Wbt (B*T, C, C) [in][out] / bbt (B*T, C): the time-conditioned parameters; W3 (J, C) / b3 (J): MLP_RL.ln3, J <= 16.  C = 64, else GPTST_ESHAPE. */
int gptst_guide_uc_floats(int N, int C);
int gptst_guide_head_fwd(const float* src, int lda, const float* w1, const float* b1, const float* Wn, const float* bn, const float* Wbt,
                         const float* bbt, const float* W3, const float* b3, float* uc, float* h1, float* h2, float* prob, int* label,
                         int BT, int N, int C, int J, void* stream);

/* "dPre chain" convention of the backward kernels (r03): the gradient that travels down the layer chain may be handed over ALREADY multiplied
 * by the LeakyReLU derivative of the activation it belongs to (dPre = dOut * lrelu'(out)).  A consumer is told so by Y == NULL (it then
 * takes its incoming gradient as dPre and never reads its own output), and a producer is told to emit that form by premul != 0: it
 * multiplies its input gradient by lrelu'(X), where X — its input, which it reads anyway — is the output of the LeakyReLU layer below.
 * Y != NULL together with premul != 0 is rejected (GPTST_EARG).
 *
 * fused hyperTem backward w.r.t. data and graph: dX = (dPre + G (*) (dPre W_bt^T)) [* lrelu'(X) if premul], dPre = dOut*lrelu'(Y) or dOut,
 * and PARTIALS of the bias and graph gradients, plain stores in a fixed order (no atomics): dbias (gptst_hypertem_ntiles(N) * B*T, C) — one
 * partial per 16-node tile — and dG (B*N, T, T) — one per sample; the consumers sum them (pool jobs nsplit, gptst_gram_bwd nsplit).
 * (The weight gradient stays in gptst_wgrad.)  C = 64.  Replaces the backward of GPTST.py:157-163. */
int gptst_hypertem_ntiles(int N);
int gptst_hypertem_bwd(const float* dOut, const float* Y, const float* X, const float* G, const float* Wbt, float* dX, float* dbias,
                       float* dG, int premul, int B, int T, int N, int C, void* stream);
/* gptst_hypertem_bwd (without dbias) AND the layer's weight + bias gradient (gptst_wgrad_colsum mode 0, pro 1, which 2 on R, dOut, Y) side
 * by side in ONE launch: the two are independent, and as separate launches their fixed dependency chains add up.
 * dWb: (gptst_wgrad_nsplit(0, B*T, N, 64) * B*T, C*C + C) rows [dW_bt | db_bt].  R == NULL: the weight-gradient workgroups rebuild
 * R_t[n,:] = sum_u G_n[t,u] X_u[n,:] from the sample's X (L2 hits: the slab workgroups of the same sample run on the same XCD) — needs
 * gptst_wgrad_nsplit(...) == 1, else GPTST_ESHAPE.  C = 64. */
int gptst_hypertem_bwd_wgrad(const float* dOut, const float* Y, const float* X, const float* G, const float* Wbt, const float* R, float* dX,
                             float* dG, float* dWb, int premul, int B, int T, int N, int C, void* stream);
/* The backward of TWO consecutive hyperTem layers (L+1 "1" above L "0", nothing in between: GPTST.py:267-268, :271 -> :454) in ONE launch (r04):
 * the slab workgroup turns dPre of layer L+1 into the input gradient times lrelu'(input) — dPre of layer L — and runs layer L on it at once;
 * grid [slab | weight gradient L+1 | weight gradient L], the last role waits (bounded, NaN on expiry) for the sample's slabs to publish dXmid.
 * dOut1 = dPre of layer L+1; X1 / X0 the layers' inputs (B,T,N,C), R1 / R0 their saved temporal mixes; -> dXmid (dPre of layer L), dX0 (times
 * lrelu'(X0)), dG1 / dG0 (B*N,T,T) per-sample partials, dWb1 / dWb0 (nsplit * B*T, C*C + C).  cnt: B 32-bit words, ZERO on entry.  C = 64. */
int gptst_hypertem_bwd_pair(const float* dOut1, const float* X1, const float* G1, const float* Wbt1, const float* R1, const float* X0,
                            const float* G0, const float* Wbt0, const float* R0, float* dXmid, float* dX0, float* dG1, float* dG0,
                            float* dWb1, float* dWb0, void* cnt, int B, int T, int N, int C, void* stream);

/* ---- cap: node x cluster soft assignment + routing + aggregation (cap.hip, cap_cross.hip), GPTST.py:100-141 ----
 * route_fwd, one workgroup per (b,t):  P = squash(X Wp^T + bp) by MFMA into LDS; dadj (BT,HS,N) = teb.adj (from gptst_poolgen_fwd);
 *   v0 = squash(softmax_h(dadj) P);  R x { c = softmax_h(b); v = squash(v0 (.) c P); b += v P^T }  (both contractions on MFMA 16x16x4);
 *   c = softmax_h(b + dadj) -> c_out (BT,HS,N);  s = c P -> (BT,HS,C).   Wp/bp = ln_p.weight ([out][in]) / bias. */
int gptst_cap_route_fwd(const float* X, const float* Wp, const float* bp, const float* dadj, float* c_out, float* s_out, int BT, int N,
                        int C, int HS, int R, void* stream);
/* cross-time hyperedges per sample (GPTST.py:125-134): v = squash(LReLU(dyn^T LReLU(dyn (s + (t+1)/12))) + s);
 * dyn (B,HT,T*HS) = time_eb_spg . t_adj (poolgen); saves Ht (B,HT,C), Rt (B,T*HS,C) for backward. */
int gptst_cap_cross_fwd(const float* s, const float* dyn, const float* tmpl, float* v, float* Ht, float* Rt, int B, int T, int C,
                        int HS, int HT, void* stream);
/* ws: device scratch of gptst_cap_cross_ws_floats() floats — 0 (ws may be NULL) while the T*HS cluster tokens of a sample fit LDS;
 * beyond that (e.g. HS = 40: 480 tokens) both calls switch to plain global-memory kernels and the backward needs B*HT*C floats. */
int gptst_cap_cross_ws_floats(int B, int T, int C, int HS, int HT);
int gptst_cap_cross_bwd(const float* dv, const float* s, const float* Rt, const float* Ht, const float* dyn, const float* tmpl,
                        float* dS, float* ddyn, float* ws, int B, int T, int C, int HS, int HT, void* stream);
/* cluster -> node scatter (GPTST.py:135): rec[bt,n,:] = sum_h c[bt,h,n] v[bt,h,:]; and its backward (dc1, dv). */
int gptst_cap_rec_fwd(const float* c, const float* v, float* rec, int BT, int N, int C, int HS, void* stream);
/* gptst_cap_cross_fwd + gptst_cap_rec_fwd in ONE launch of B*T workgroups: every (b,t) workgroup rebuilds the sample's Ht (repeated by
 * the T workgroups of a sample) and Rt / v of its own HS tokens, then scatters rec[bt] = c[bt]^T v[bt].  Bit-identical to the two launches.
 * C = 64 and the sample's tokens + c[bt] within 80 KB of LDS, else GPTST_ESHAPE.  GPTST.py:125-135. */
int gptst_cap_cross_rec_fwd(const float* s, const float* dyn, const float* tmpl, const float* c, float* v, float* Ht, float* Rt, float* rec,
                            int B, int T, int N, int C, int HS, int HT, void* stream);
int gptst_cap_rec_bwd(const float* drec, const float* c, const float* v, float* dc1, float* dv, int BT, int N, int C, int HS,
                      void* stream);
/* backward through s = c P, c = softmax_h(b + dadj) (routing logits b are detached, GPTST.py:108-109) and the squash:
 * dY (BT*N,C) = grad of X Wp^T + bp;  dlogit (BT,HS,N) = grad of dadj. */
int gptst_cap_route_bwd(const float* X, const float* Wp, const float* bp, const float* c, const float* dc1, const float* dS,
                        float* dY, float* dlogit, int BT, int N, int C, int HS, void* stream);
/* gptst_cap_cross_bwd + gptst_cap_route_bwd in ONE launch of B*T workgroups: the backward of the cross-time block (GPTST.py:125-134) runs as a
 * prologue of every (b,t) workgroup (the part that needs the whole sample is repeated by its T workgroups), dS stays in LDS.
 * dv (B, T*HS, C): gradient of v;  -> dY, dlogit as gptst_cap_route_bwd, ddyn (B, HT, T*HS).  C = 64, else GPTST_ESHAPE.
 * r04 — dS_ws (B*T, HS, C) scratch + flags (4 B 32-bit words, ZERO on entry): both given -> the cross-time backward is a ROLE of the launch: 4 B extra
 * workgroups do it (four per sample, three time steps each) and publish dS (write-through stores + one flag per sample) while the B*T routing workgroups rebuild their
 * capsule tile, which does not depend on dS, and pick dS up behind it (a bounded wait; on expiry dS is poisoned with NaN: a lost hand-off ends the run loudly).
 * Either NULL: every (b,t) workgroup repeats the cross-time backward as a prologue (r03). */
int gptst_cap_cross_route_bwd(const float* X, const float* Wp, const float* bp, const float* c, const float* dc1, const float* dv,
                              const float* s, const float* Rt, const float* Ht, const float* dyn, const float* tmpl, float* dY,
                              float* dlogit, float* ddyn, float* dS_ws, void* flags, int B, int T, int N, int C, int HS, int HT, void* stream);
/* r05 — gptst_cap_cross_route_bwd + gptst_linear_bwd in ONE launch: each (b,t) workgroup goes on from its dY tile (kept in LDS; no dY tensor exists) to
 * the backward of cap's entry Linear (GPTST.py:102) and the layer's residual branch (:139-141):
 *   out == NULL: dX = dY Wp + dPre (the incoming gradient already is dPre), times lrelu'(X) when premul;   out given: dX = dY Wp + dPre*lrelu'(out).
 *   dWp (B*T, C*C) [out][in] and dbp (B*T, C): ONE partial per (b,t) — the caller's reduction sums B*T rows.
 * dlogit, ddyn, dS_ws, flags as gptst_cap_cross_route_bwd.  C = 64, else GPTST_ESHAPE (use the two calls). */
int gptst_cap_cross_route_lin_bwd(const float* X, const float* Wp, const float* bp, const float* c, const float* dc1, const float* dv,
                                  const float* s, const float* Rt, const float* Ht, const float* dyn, const float* tmpl,
                                  const float* dPre, const float* out, int premul, float* dX, float* dWp, float* dbp, float* dlogit,
                                  float* ddyn, float* dS_ws, void* flags, int B, int T, int N, int C, int HS, int HT, void* stream);
/* r05, late — gptst_cap_cross_route_lin_bwd followed by gptst_pool_jobs(njobs, ...) with gradient-reduction jobs (kinds 1 and 2 only), in ONE launch where the
 * role form serves (dS_ws and flags given, not the deterministic mode): the jobs run as further role workgroups behind the routing workgroups, on the CUs and the
 * HBM bandwidth this launch leaves idle (384 routing workgroups on 256 CUs at ~2.3 TB/s).  The jobs' inputs must have been written by EARLIER launches of the
 * stream and nothing in this launch reads their outputs (the steppers: the decoder's weight-gradient reductions under the encoder's routing backward).
 * Otherwise exactly the two calls.  Same results either way (kind-2 outputs are float atomics as in gptst_pool_jobs). */
/* 1 when gptst_cap_cross_route_lin_bwd at this shape takes the role form that also carries jobs (every workgroup resident: B*T + 4 B <= 512, <= 80 KB of LDS) */
int gptst_cap_route_roles_ok(int B, int T, int N, int C, int HS, int HT);
int gptst_cap_cross_route_lin_bwd_jobs(const float* X, const float* Wp, const float* bp, const float* c, const float* dc1, const float* dv,
                                       const float* s, const float* Rt, const float* Ht, const float* dyn, const float* tmpl,
                                       const float* dPre, const float* out, int premul, float* dX, float* dWp, float* dbp, float* dlogit,
                                       float* ddyn, float* dS_ws, void* flags, int B, int T, int N, int C, int HS, int HT,
                                       int njobs, const int* jkind, const void* const* jemb, const void* const* jx, const void* const* jpool,
                                       const void* const* jout, const int* jR, const int* jK, const int* jcols, const int* jnsplit, const int* jldx,
                                       void* stream);
/* r06 NODE HALVES.  The (b,t)-grouped cap kernels run B*T = 384 workgroups on the 256 CUs of an MI355X at two per CU: half the CUs get two units, the rest
 * one, and the launch lasts as long as the former (the reference has no such notion: GPTST.py:100-141 is a chain of whole-tensor einsums).  Every step of
 * the routing backward is local to a 16-node tile, so the LAST nsplit (b,t) can be cut into two node halves with a workgroup each (B*T - nsplit whole
 * units + 2 nsplit halves: at B*T = 1.5 x CUs one whole unit and one half per CU).
 * MEASURED AND NOT ADOPTED (profiles/r06_node_halves.txt: a half lasts as long as a whole unit — the workgroup is a latency chain, not a throughput item):
 * gptst_cap_split_units returns 0 unless a test / benchmark turns the policy on (gptst_tune(25, -1): B*T - CUs where CUs < B*T <= 1.5 CUs, C = 64, N >= 32) — what a caller passes to
 * gptst_cap_cross_route_lin_bwd_split, which is gptst_cap_cross_route_lin_bwd_jobs (njobs may be 0) with dWp (B*T + nsplit, C*C) and dbp (B*T + nsplit, C):
 * a half writes a partial row of its own (rows B*T - nsplit + 2k, + 2k + 1 are the halves of (b,t) = B*T - nsplit + k).  Any 0 <= nsplit <= B*T is valid;
 * the results do not depend on it beyond the summation order of the caller's reduction over the partial rows. */
int gptst_cap_split_units(int BT, int N, int C, int HS);
int gptst_cap_cross_route_lin_bwd_split(const float* X, const float* Wp, const float* bp, const float* c, const float* dc1, const float* dv,
                                        const float* s, const float* Rt, const float* Ht, const float* dyn, const float* tmpl,
                                        const float* dPre, const float* out, int premul, float* dX, float* dWp, float* dbp, float* dlogit,
                                        float* ddyn, float* dS_ws, void* flags, int B, int T, int N, int C, int HS, int HT, int nsplit,
                                        int njobs, const int* jkind, const void* const* jemb, const void* const* jx, const void* const* jpool,
                                        const void* const* jout, const int* jR, const int* jK, const int* jcols, const int* jnsplit, const int* jldx,
                                        void* stream);

/* ---- cap for node counts whose (b,t) capsule matrix does not fit LDS (cap_big.hip; BASELINE config 5: N = 4096, C = 128) ----
 * gptst_cap_fits_lds() == 0 -> the host composes the same algebra from these streaming kernels (ops.py: cap_route_fwd/bwd, cap_rec_*):
 * P = squash(X Wp^T + bp) via gptst_apply + capbig_squash_rows;  cs = softmax_h(use_bl*bl + use_l0*l0)  (all (BT,HS,N));
 * type1: S (BT,HS,C) = cs . P  — the ONLY sum over nodes, i.e. the all-reduce point of a node-sharded run;
 * post: 0 out = S, 1 out = squash(S), 2 out = squash(V0 (.) S);  type2: bl += V . P^T;  rec_fwd / rec_bwd_dc: cluster -> node scatter
 * and the c-gradient of it (dv = type1(c, drec));  route_bwd_rows: backward of gptst_cap_route_bwd given Y = X Wp^T + bp. */
int gptst_cap_fits_lds(int N, int C, int HS);
int gptst_capbig_squash_rows(float* Y, long rows, int C, void* stream);
int gptst_capbig_softmax(const float* bl, const float* l0, float* cs, int BT, int HS, int N, int use_bl, int use_l0, void* stream);
int gptst_capbig_type1(const float* cs, const float* P, float* S, int BT, int HS, int N, int C, void* stream);
int gptst_capbig_post(const float* S, const float* V0, float* out, long rows, int C, int post, void* stream);
int gptst_capbig_type2(const float* V, const float* P, float* bl, int BT, int HS, int N, int C, void* stream);
int gptst_capbig_rec_fwd(const float* c, const float* v, float* rec, int BT, int HS, int N, int C, void* stream);
int gptst_capbig_rec_bwd_dc(const float* drec, const float* v, float* dc1, int BT, int HS, int N, int C, void* stream);
int gptst_capbig_route_bwd_rows(const float* Y, const float* c, const float* dc1, const float* dS, float* dY, float* dlogit, int BT,
                                int HS, int N, int C, void* stream);

/* ---- streaming cap, second generation (capflow.hip): one fused MFMA pass over the capsule matrix per routing iteration ----
 * Same algebra as above for HS <= 16, C in {64,128} (gptst_capflow_supported); sums over nodes leave the kernels as partials per
 * gptst_capflow_nparts(N) node chunks and are folded in index order by gptst_capflow_post (no atomics):
 * squash:  P = squash(Y) row-wise; c0 = softmax_h(dadj); part (BT,nparts,HS+1,C) = [c0^T P ; colsum P]  (colsum = the first routing
 *          iteration, whose coefficients are uniform);
 * route:   L = V ? rows . V^T : 0;  b = L + bl_in;  bl_out <- b;  cs = c_in ? c_in : softmax_h(b + l0);  c_out <- cs;
 *          part (BT,nparts,HS,C) = cs^T . rows   (NULL = operand absent).  Routing iteration: (P, v, b);  last step: (P, v, b, l0 = dadj,
 *          c_out = c);  backward of rec = c^T v: rows = drec, V = v, bl_out = dc1, c_in = c, fold of part = dv;
 * post:    part (BT,nparts,prow,C) -> mode 0 (prow = HS+1): V0 = squash(S0), Vout = squash(V0 (.) colsum/HS) (if given);
 *          mode 1: Vout = squash(V0 (.) S);  mode 2: Vout = S;  mode 3: Vout (BT,prow,C) = plain fold (a node-sharded run all-reduces
 *          it and calls post again with nparts = 1);
 * rec_fwd: rec (BT*N,C) = c^T v;  route_bwd: as gptst_capbig_route_bwd_rows. */
int gptst_capflow_supported(int HS, int C);
int gptst_capflow_nparts(int N);
int gptst_capflow_squash(const float* Y, const float* dadj, float* P, float* part, int BT, int HS, int N, int C, void* stream);
int gptst_capflow_route(const float* rows, const float* V, const float* bl_in, float* bl_out, const float* l0, const float* c_in,
                        float* c_out, float* part, int BT, int HS, int N, int C, void* stream);
int gptst_capflow_post(const float* part, int nparts, int prow, float* V0, float* Vout, int mode, int BT, int HS, int C, void* stream);
int gptst_capflow_rec_fwd(const float* c, const float* v, float* rec, int BT, int HS, int N, int C, void* stream);
int gptst_capflow_route_bwd(const float* Y, const float* c, const float* dc1, const float* dS, float* dY, float* dlogit, int BT,
                            int HS, int N, int C, void* stream);

/* ---- evaluation metrics of Trainer.test (metrics.hip), reference model/BasicTrainer.py:209-248 + lib/metrics.py:11-18,38-43,52-86 ----
 * Accumulates, over one batch, the sums the per-horizon MAE / RMSE / MAPE / CORR need (doubles; caller zeroes them once per evaluation):
 * sums_t (T,5) = [n1, sum|e|, sum e^2, n2, sum|e/y|], sums_tn (T,N,6) = [K, sum p, sum y, sum p^2, sum y^2, sum p y];
 * p = (out*m)*sigma+mu, y = (label*m)*sigma+mu with m = 1 - vis (pretrain mode, :229-235); vis == NULL -> m = 1. */
int gptst_metrics_accum(const float* out, const float* src, int lda, const float* vis, float sigma, float mu, int has_mae_thresh,
                        float mae_thresh, float mape_thresh, int B, int T, int N, int D, double* sums_t, double* sums_tn, void* stream);

/* ---- mask generation, integer work, bit-exact given noise/labels/class order (masksel.hip), GPTST.py:314-323,344-413 ----
 * Masks are fp32 {0,1} arrays, 1 = visible, 0 = masked.  Top-k = radix select on the float bits, 11/11/10-bit digits (ties at
 * rank k -> lowest index).  Up to 2^13 cells the whole generation (class histogram and roles, both selections, mask writes) is ONE
 * launch of one 1024-thread workgroup; beyond, one launch per digit + one to write the mask, 64 workgroups each (the adaptive phase's
 * first mask write also histograms the first digit of the second selection). */
int gptst_mask_ws_bytes(void);   /* device scratch (ws) needed by the two selections below */
/* ws_zeroed != 0: the caller hands ws over all-zero (e.g. as part of a scratch region it clears once per step) — saves the zeroing launch.
 * ws is left dirty. */
int gptst_mask_random(const float* noise, int M, int k, float* mask, void* ws, int ws_zeroed, void* stream);
/* label[i] = argmax_h prob[i,h] (int32), counts[h] (int32, zeroed here) — replaces sort(..)[..., 0] (:344-345). */
int gptst_mask_labels(const float* prob, int rows, int HS, int* label, int* counts, void* stream);
/* adaptive phase: device-side class selection (:356-384) + two selections (:386-407) + product (:410-413).
 * list_c: shuffled class order (int32[HS]); nums: {adaptive_mask_num, random_mask_num} int32[2] on the device;
 * m_ada / m_rnd (M) are the partial masks, mask (M*base) the final one.
 * counts may be NULL: the class histogram is then taken from the labels here (inside the single launch for M <= 2^13, by one more
 * small launch beyond). */
int gptst_mask_adaptive(const int* label, const int* counts, const int* list_c, const int* nums, const float* noise_a,
                        const float* noise_r, int ada_all, int M, int HS, int base, float* m_ada, float* m_rnd, float* mask,
                        void* ws, int ws_zeroed, void* stream);

/* r04 — mask generation for noise on the 2^-24 lattice (every value k * 2^-24, 0 <= k < 2^24: what the step's Philox draws and torch.rand
 * produce): the radix select runs on the integers k with TWO uniform 12-bit digits instead of three float-bit digits — one launch less per
 * selection (adaptive phase 6 launches instead of 8); up to 8192 cells the whole generation is ONE launch of one workgroup.  Same results as
 * gptst_mask_random / gptst_mask_adaptive bit for bit (ties at the threshold in index order).  The lattice is CHECKED on the device: any other
 * noise value poisons the outputs with NaN.  ws / ws_zeroed / counts as in the calls above; m_ada / m_rnd must be given beyond 8192 cells. */
int gptst_mask_random_u24(const float* noise, int M, int k, float* mask, void* ws, int ws_zeroed, void* stream);
int gptst_mask_adaptive_u24(const int* label, const int* counts, const int* list_c, const int* nums, const float* noise_a, const float* noise_r,
                            int ada_all, int M, int HS, int base, float* m_ada, float* m_rnd, float* mask, void* ws, int ws_zeroed, void* stream);
/* r05 — gptst_pool_jobs with njobs generation jobs (kind[j] 0: out_j (R_j, cols_j) = emb_j (R_j, K_j) @ pool_j (K_j, cols_j), or 3: the temporal graphs of
 * gptst_pool_jobs; kind NULL: all 0; no gradient kinds) followed by gptst_mask_random_u24
 * (adaptive == 0: noise_a is the noise, k the number of cells to drop) or gptst_mask_adaptive_u24 (adaptive != 0; k unused) — in ONE launch when the mask
 * takes the cooperative form (gptst_mask_cooperative, 8192 < M <= 1048576, ws given) and every forward job has cols % 4 == 0: the (at most 128) mask workgroups are
 * latency-bound on as many CUs, the jobs are write-bound on all of them, and neither depends on the other (the steppers: the generated parameters of the
 * two STHCNs next to the mask that the guide's output selects).  Otherwise exactly those two calls.  Same results bit for bit either way. */
int gptst_mask_u24_fwd_jobs(int adaptive, const int* label, const int* counts, const int* list_c, const int* nums, const float* noise_a,
                            const float* noise_r, int ada_all, int M, int HS, int base, int k, float* m_ada, float* m_rnd, float* mask, void* ws,
                            int ws_zeroed, int njobs, const int* kind, const void* const* emb, const void* const* pool, const void* const* out,
                            const int* R, const int* K, const int* cols, void* stream);

/* ---- thin projections (small.hip) ------------------------------------------------------------------------
 * lin_in: Y[i,:] = sum_j a'[i,j] W(:,j) + b, a' = mask ? (mask[i,j] ? a[i*lda+j] : fill) : a;  wlayout 0: W[c*J+j], 1: W[j*C+c].
 *   (dim_in_flow on the masked source, GPTST.py:416-418; MLP_RL.ln1 :22; data-gradients of rowdot)
 * rowdot: Z[i,j] = X[i,:].W[j,:] + b[j] (+ softmax over j)   (dim_flow_out :455; MLP_RL.ln3 + softmax :33,:332)
 * rowouter: out(j,c) += sum_i a'[i,j] X[i,c] (olayout 0: out[c*J+j], 1: out[j*C+c]); csum[c] += sum_i X[i,c];
 *   asum[j] += sum_i a'[i,j]    (weight / bias gradients of both) */
int gptst_lin_in(const float* a, int lda, const float* mask, float fill, const float* W, int wlayout, const float* b, float* Y,
                 int rows, int J, int C, void* stream);
/* label (optional, int32 per row): argmax_j Z[i,j], first maximum — the cluster label of the adaptive mask (GPTST.py:344-345) */
int gptst_rowdot(const float* X, const float* W, const float* b, float* Z, int rows, int J, int C, int do_softmax, int* label,
                 void* stream);
/* r04 — the gate of the downstream front end (reference model/Model.py:5-18 Fusion, :106 lin_test) in one launch:
 *   x_t = flow . Wt^T + bt  (flow: `base` values per row of src at stride lda);  z = sigmoid(F Ws^T + bs + x_t Wh^T + bh);
 *   out = (z F + (1 - z) x_t) Wo^T + bo.      F, out, z: (rows, C); weights as nn.Linear stores them ([out][in]); z may be NULL (inference).
 * gptst_fusion_gate_bwd: the backward's data path — dpre = dHm (F - x_t) z (1 - z) with dHm = dOut Wo (gradient of both gate pre-activations),
 * dxd = dHm (1 - z), and Hm, xt re-formed as operands of the weight gradients (gptst_wgrad_colsum / gptst_apply do those: gpt-st_amd/fusion.py).
 * C = 64 and base <= 4, else GPTST_ESHAPE. */
int gptst_fusion_gate_fwd(const float* F, const float* src, int lda, int base, const float* Ws, const float* bs, const float* Wh,
                          const float* bh, const float* Wo, const float* bo, const float* Wt, const float* bt, float* out, float* z,
                          int rows, int C, void* stream);
int gptst_fusion_gate_bwd(const float* dOut, const float* F, const float* z, const float* src, int lda, int base, const float* Wo,
                          const float* Wt, const float* bt, float* dpre, float* dxd, float* Hm, float* xt, int rows, int C, void* stream);
/* gptst_fusion_gate_bwd when the embedding F is trained too (fine-tuning the encoder): the same four tensors, bit-identical, and in the same
 * launch dF (rows, C) = dHm z + dpre Ws, the gradient of F through the blend and through HS_fc.  C = 64 and base <= 4, else GPTST_ESHAPE. */
int gptst_fusion_gate_bwd_df(const float* dOut, const float* F, const float* z, const float* src, int lda, int base, const float* Wo,
                             const float* Wt, const float* bt, const float* Ws, float* dpre, float* dxd, float* Hm, float* xt, float* dF,
                             int rows, int C, void* stream);
/* ---- the downstream STGCN predictor (stgcn.hip; reference model/STGCN/stgcn.py, gpt-st_amd/predictors/stgcn_hip.py) ----------------------
 * Channels-last throughout: an activation is (rows = B*T*N, C), a temporal tap is a row offset of dt*N rows, nothing is permuted.
 * act: 0 none, 1 relu, 2 sigmoid, 3 GLU.  Widths are multiples of 16, else GPTST_ESHAPE.
 * tapgemm: Y (rows, co) = act(sum_j X[row + dt_j N][0..ci) W_j + bias + res): W (co or, GLU, 2 co rows; ntap*ci columns, tap-major),
 *   ntap <= 4 taps of time offsets dt_j (a tap outside [0, T) is zero padding and is not read), res = R[row][ch] for ch < res_w (row stride
 *   ldr; res_w = 0: none).  GLU: Y = (P + bias + res) sigmoid(Q + bias), P = W rows [0, co), Q = rows [co, 2 co); S, A (rows, co; both or
 *   neither) keep sigmoid(Q) and P + bias + res for the backward.  ntap*ci <= 1024.
 * gate_bwd: dPre from dOut: relu / sigmoid from the layer's output `out`; GLU from S, A -> dPre (rows, 2 co) = [dOut S | dOut A S (1 - S)].
 * wgrad: part (nsplit, cw, ntap*ci) = row-split partials of D^T X_shift (D (rows, cw) = dPre; X, ci, taps as in tapgemm), bpart
 *   (nsplit, cw; may be NULL) = those of the column sums of D; the caller sums the splits (fixed order, no atomics).
 * nodemix: per (b,t) unit of N rows, with L (ks, Np, Np) zero-padded to Np = 16 ceil(N/16):  reduce = 0: Out (rows, ks*c), Out[:, k c + ch] =
 *   (L_k In)[:, ch], In (rows, c);  reduce = 1: Out (rows, c) = sum_k L_k In[:, k c ..] + R, In (rows, ks*c), R (rows, c) or NULL.
 * ln_fwd / ln_bwd / ln_bwd_param: LayerNorm over the M = N*C values of a unit (gamma, beta: M values): Y, and mean, rstd (units; may both
 *   be NULL);  dX;  pg, pb (nsplit, M) = unit-split partials of dgamma, dbeta. */
int gptst_stgcn_tapgemm(const float* X, int ldx, int ci, int ntap, int dt0, int dt1, int dt2, int dt3, const float* W, const float* bias,
                        const float* R, int ldr, int res_w, float* Y, int co, float* S, float* A, int act, int rows, int T, int N,
                        void* stream);
int gptst_stgcn_gate_bwd(const float* dOut, const float* out, const float* S, const float* A, float* dPre, int act, int rows, int co,
                         void* stream);
int gptst_stgcn_wgrad_nsplit(int rows, int cw, int Ktot);
int gptst_stgcn_wgrad(const float* D, int cw, const float* X, int ldx, int ci, int ntap, int dt0, int dt1, int dt2, int dt3, float* part,
                      float* bpart, int nsplit, int rows, int T, int N, void* stream);
int gptst_stgcn_nodemix(const float* L, int Np, int ks, const float* In, float* Out, const float* R, int c, int reduce, int units, int N,
                        void* stream);
int gptst_stgcn_ln_fwd(const float* X, const float* gamma, const float* beta, float* Y, float* mean, float* rstd, int units, int M,
                       float eps, void* stream);
int gptst_stgcn_ln_bwd(const float* dY, const float* X, const float* gamma, const float* mean, const float* rstd, float* dX, int units,
                       int M, void* stream);
int gptst_stgcn_ln_nsplit(int units);
int gptst_stgcn_ln_bwd_param(const float* dY, const float* X, const float* mean, const float* rstd, float* pg, float* pb, int nsplit,
                             int units, int M, void* stream);
/* ---- the downstream TGCN predictor's recurrence (tgcn.hip; reference model/TGCN/TGCN.py:70-91, gpt-st_amd/predictors/tgcn_hip.py) -------------
 * Per step t: [r, u] = sigmoid(L [x_t, h] W0 + b0), c = tanh(L [x_t, r h] W1 + b1), h' = u h + (1 - u) c.  The x_t halves (Gx0 = L X W0[:C] + b0,
 * Gx1 likewise) and every weight / input gradient are hoisted onto gptst_stgcn_nodemix / tapgemm / wgrad; these four launches are the h chain.
 * A "step" tensor is (B*N, Hp), row b N + n; a "seq" tensor is (B*T*N, width), row (b T + t) N + n.  Hp = rnn_units zero-padded to a multiple of
 * 16 (16..128, else GPTST_ESHAPE); L / LT (Np, Np) zero-padded to Np = 16 ceil(N/16).  Each launch computes M = L[rows, :] In_b per batch element,
 * P = M Wt^T with Wt (outputs, K) row-major, and an epilogue.  tiles: 16-node tiles per workgroup, 1 or 2; 0 = chosen from B and N.
 * fwd_gates: In = h;  W0h (2 Hp, Hp);  Gx0 (seq, 2 Hp) -> u, q = r h (step), and when not NULL r (step) and z[seq row][zoff + col] = M (ld ldz).
 * fwd_state: In = q;  W1h (Hp, Hp);  Gx1 (seq, Hp) -> h_out = u h + (1 - u) c (step; may be h), and when not NULL c (step) and z as above.
 * bwd_cand:  In = dpre1 = dh (1 - u)(1 - c^2) formed on load, -> dpre1 (seq, Hp);  W1hT (Hp, Hp) = W1h^T;  -> dpre0 (seq, 2 Hp) =
 *            [dq h r (1 - r) | dh (h - c) u (1 - u)], dh_part = dh u + dq r (step; not dh);  h = the step's INPUT state.
 * bwd_state: In = dpre0 (seq, 2 Hp);  W0hT (Hp, 2 Hp) = W0h^T  -> dh_out = dh_part + P (step).
 * lds_bytes: the dynamic LDS of the widest of the four at this shape (above 160 KB they return GPTST_ESHAPE). */
int gptst_tgcn_lds_bytes(int N, int Hp, int B);
int gptst_tgcn_fwd_gates(const float* L, int Np, const float* W0h, const float* h, const float* Gx0, float* u, float* r, float* q,
                         float* z, int ldz, int zoff, int B, int T, int N, int Hp, int t, int tiles, void* stream);
int gptst_tgcn_fwd_state(const float* L, int Np, const float* W1h, const float* q, const float* Gx1, const float* u, const float* h,
                         float* h_out, float* c, float* z, int ldz, int zoff, int B, int T, int N, int Hp, int t, int tiles,
                         void* stream);
int gptst_tgcn_bwd_cand(const float* LT, int Np, const float* W1hT, const float* dh, const float* u, const float* c, const float* r,
                        const float* h, float* dpre1, float* dpre0, float* dh_part, int B, int T, int N, int Hp, int t, int tiles,
                        void* stream);
int gptst_tgcn_bwd_state(const float* LT, int Np, const float* W0hT, const float* dpre0, const float* dh_part, float* dh_out, int B,
                         int T, int N, int Hp, int t, int tiles, void* stream);
/* ---- the downstream MTGNN predictor (mtgnn.hip; reference model/MTGNN/MTGNN.py, gpt-st_amd/predictors/mtgnn_hip.py) ------------------------
 * Rows (b, t, n), channels last, as above; a tensor's time length is its frame.  Widths are multiples of 16, else GPTST_ESHAPE.
 * tapgemm: Y (B*Tdst*N, co)[b, to, n] = epi(sum_j X[b, to + offs[j], n][0..ci) W_j + bias): X (B*Tsrc*N rows, row stride ldx), ntap <= 32 taps
 *   (host array offs; a tap whose source time falls outside [0, Tsrc) is not read), W (co or, gated, 2 co rows; ntap*ci columns, tap-major), any
 *   K (walked in chunks).  XM (X's layout, or NULL) multiplies the operand.  gated = 0: epi(v) = (v + R[b, to + roff, n][ch]) OM, R of frame Tr
 *   and row stride ldr read where 0 <= to + roff < Tr (NULL: none; R may be Y when Tr == Tdst and roff == 0: accumulation), OM (rows, co; NULL: 1).
 *   gated = 1: Y = tanh(P + bias) sigmoid(Q + bias) OM, P = W rows [0, co), Q = rows [co, 2 co); Tn, S (rows, co; both or neither) keep the tanh
 *   and the sigmoid.  The data backward is the same call: X = dPre, taps -offs[j], W = [W_j^T]_j, frames swapped, R = a second gradient.
 * gate_bwd: dPre (rows, 2 co) = [dG OM S (1 - Tn^2) | dG OM Tn S (1 - S)].
 * wgrad: part (nsplit, cw, ntap*ci) = row-split partials of sum_rows D[b, to, n]^T (X XM)[b, to + offs[j], n], D (B*Tdst*N, cw); bpart (nsplit, cw;
 *   may be NULL) = those of the column sums of D; nsplit = gptst_stgcn_wgrad_nsplit(B*Tdst*N, cw, ntap*ci); the caller sums the splits.
 * graphgrad: part (nsplit, ks, N, N) = unit-split partials of dM_k[v][w] = sum_{unit, ch} D[unit N + v][dcol0 + k c + ch] X[unit N + w][ch]: the
 *   gradient of gptst_stgcn_nodemix (reduce = 0: D = dOut, X = In) with respect to L_k, unpadded; units of exactly N rows. */
int gptst_mtgnn_tapgemm(const float* X, int ldx, int ci, const float* XM, int ntap, const int* offs, const float* W, const float* bias,
                        const float* R, int ldr, int Tr, int roff, const float* OM, float* Y, int co, float* Tn, float* S, int gated,
                        int B, int Tsrc, int Tdst, int N, void* stream);
int gptst_mtgnn_gate_bwd(const float* dG, const float* Tn, const float* S, const float* OM, float* dPre, int rows, int co, void* stream);
int gptst_mtgnn_wgrad(const float* D, int cw, const float* X, int ldx, int ci, const float* XM, int ntap, const int* offs, float* part,
                      float* bpart, int nsplit, int B, int Tsrc, int Tdst, int N, void* stream);
int gptst_mtgnn_graphgrad_nsplit(int units, int N, int ks);
int gptst_mtgnn_graphgrad(const float* D, int ldd, int dcol0, const float* X, int ldx, int c, int ks, float* part, int nsplit, int units,
                          int N, void* stream);
/* ---- the downstream ASTGCN predictor (astgcn.hip; reference model/ASTGCN/ASTGCN.py, gpt-st_amd/predictors/astgcn_hip.py) --------------------
 * Rows as for STGCN: (b T + t) N + n.  Tp (ks, Np, Np): the Chebyshev polynomials zero-padded to Np = 16 ceil(N / 16); S (B, N, N): the spatial
 * attention of every sample, unpadded; ks <= 3; c a multiple of 16.  The masked graph T_k * S_b is formed in LDS and never written.
 * attmix, reduce = 0: In (rows, c) -> Out (rows, ks c), Out[(b,t,n), k c + ch] = sum_m T_k[m,n] S[b,m,n] In[(b,t,m), ch];
 *         reduce = 1: In (rows, ks c) -> Out (rows, c), Out[(b,t,m), ch] = sum_k sum_n T_k[m,n] S[b,m,n] In[(b,t,n), k c + ch] + R (R may be NULL).
 *         ESHAPE when Np > 320 (the masked tiles and the slab, Np (20 ks + 68) floats, fit 160 KB of LDS up to there).
 * attgrad: dS (B, N, N), dS[b,m,n] = sum_k T_k[m,n] sum_{t,ch} X[(b,t,m), ch] G[(b,t,n), k c + ch]; X (rows, c), G (rows, ks c).
 * rowln_*: LayerNorm over the c <= 128 values of each row; mean, rstd (rows; both NULL: not kept); bwd_param: pg, pb (nsplit, c) = row-split
 *   partials of dgamma, dbeta in a fixed order, nsplit = gptst_astgcn_rowln_nsplit(rows); the caller sums the splits. */
int gptst_astgcn_attmix(const float* Tp, int Np, int ks, const float* S, const float* In, float* Out, const float* R, int c, int reduce,
                        int B, int T, int N, void* stream);
int gptst_astgcn_attgrad(const float* Tp, int Np, int ks, const float* X, const float* G, float* dS, int c, int B, int T, int N,
                         void* stream);
int gptst_astgcn_rowln_fwd(const float* X, const float* gamma, const float* beta, float* Y, float* mean, float* rstd, long rows, int c,
                           float eps, void* stream);
int gptst_astgcn_rowln_bwd(const float* dY, const float* X, const float* gamma, const float* mean, const float* rstd, float* dX, long rows,
                           int c, void* stream);
int gptst_astgcn_rowln_nsplit(long rows);
int gptst_astgcn_rowln_bwd_param(const float* dY, const float* X, const float* mean, const float* rstd, float* pg, float* pb, int nsplit,
                                 long rows, int c, void* stream);
/* ---- the downstream STSGCN predictor (stsgcn.hip; reference model/STSGCN/STSGCN.py, gpt-st_amd/predictors/stsgcn_hip.py) --------------------
 * A layer over T frames has W = T - 2 windows.  Row layouts: frames (b, t, n); expanded (b, w, k, n), k = 0..2, block (w, k) standing for
 * frame w + k; middle (b, w, n).  L (Np, Np): A^ (the adjacency with a unit diagonal) — or its transpose for the adjoints — zero-padded to
 * Np = 16 ceil(N / 16) <= 448 (GPTST_ESHAPE beyond).  Widths are multiples of 16.
 * mix: mix(S)_k = L S_k + [k >= 1] S_{k-1} + [k <= 1] S_{k+1}, the (3N, 3N) localized adjacency never formed.  mode 0 frames -> expanded
 *   (block (w, k) reads frame w + k), 1 expanded -> expanded, 2 expanded -> middle (k = 1 only), 3 middle -> expanded (the adjoint of 2: block 1 =
 *   L In, blocks 0 and 2 = In), 4 expanded -> frames (the adjoint of 0: frame t gathers the blocks with w + k = t, k ascending).  In != Out.
 * wingemm: Y[(b, w, r)] = act(X[(b, w, r)] Wt[w]^T + bias[w]) over B W groups of R rows, R = 3N (expanded; 4N: the four-frame windows of STFGNN,
 *   below) or N (middle); Wt (W, cw, ci), bias
 *   (W, cw), cw = 2 co (act 3, GLU) or co (act 0); shared != 0: ONE weight (cw, ci) for all windows.  GLU: S = sigma(Q) and A = P + bias when not
 *   NULL.  best (B W N, co) not NULL (GLU): the running max on the middle block (rows N .. 2N of a group of 3N or 4N; all of a group of N) —
 *   operation opj = 0 writes, a later one replaces where strictly greater — and which (int32, same shape; may be NULL) the operation that holds it.
 * gate_bwd: dPre (rows, 2 co) = [g S | g A S (1 - S)] with g = up (rows, co; NULL: 0) + dBest [which == opj] on the middle block.
 * winwgrad: part (W, nsplit, cw, ci) = row-split partials of D[window]^T X[window], bpart (W, nsplit, cw) (or NULL) of D's column sums, in a
 *   fixed order; nsplit = gptst_stsgcn_winwgrad_nsplit(B R, cw, ci, W); the caller sums the splits. */
int gptst_stsgcn_mix(const float* L, int Np, const float* In, float* Out, int c, int mode, int B, int T, int N, void* stream);
int gptst_stsgcn_wingemm(const float* X, int ci, const float* Wt, const float* bias, int shared, float* Y, int co, float* S, float* A, int act,
                         float* best, int* which, int opj, int B, int W, int R, int N, void* stream);
int gptst_stsgcn_gate_bwd(const float* up, const float* dBest, const int* which, int opj, const float* S, const float* A, float* dPre, int B,
                          int W, int R, int N, int co, void* stream);
int gptst_stsgcn_winwgrad_nsplit(int wrows, int cw, int ci, int W);
int gptst_stsgcn_winwgrad(const float* D, int cw, const float* X, int ci, float* part, float* bpart, int nsplit, int B, int W, int R,
                          void* stream);
/* ---- the downstream STFGNN predictor (stfgnn.hip; reference model/STFGNN/STFGNN.py, gpt-st_amd/predictors/stfgnn_hip.py) --------------------
 * A layer over T frames has W = T - 3 windows of four frames.  Row layouts: frames (b, t, n); expanded (b, w, k, n), k = 0..3, block (w, k)
 * standing for frame w + k; middle (b, w, n).  S, D (Np, Np): S^ (the spatial adjacency with a unit diagonal) and the temporal graph D (which
 * has one) — or their transposes for the adjoints — zero-padded to Np = 16 ceil(N / 16) <= 448 (GPTST_ESHAPE beyond, nothing written).
 * mix: the product with the (4N, 4N) fusion graph, never formed: mix(X)_0 = mix(X)_3 = D (X_0 + X_3) + X_1 + X_2, mix(X)_k = S X_k + the
 *   other three blocks for k = 1, 2.  mode 0 frames -> expanded, 1 expanded -> expanded (its own adjoint with the transposed graphs),
 *   2 expanded -> middle (k = 1 only; D unused), 3 middle -> expanded (the adjoint of 2: block 1 = S In, blocks 0, 2, 3 = In), 4 expanded ->
 *   frames (the adjoint of 0: the two products of a frame in one workgroup, the gather order fixed: csrc/stfgnn.hip).  In != Out.
 * The GEMM grouped by window, its gate backward and weight gradient are gptst_stsgcn_wingemm / _gate_bwd / _winwgrad with R = 4N; the gated
 * temporal branch is gptst_mtgnn_tapgemm (gated, offsets 0 and 3) with gptst_mtgnn_gate_bwd / gptst_mtgnn_wgrad. */
int gptst_stfgnn_mix(const float* S, const float* D, int Np, const float* In, float* Out, int c, int mode, int B, int T, int N, void* stream);

/* ---- the downstream STGODE predictor (stgode.hip; reference model/STGODE/STGODE.py, odegcn.py, gpt-st_amd/predictors/stgode_hip.py) ----------
 * Rows (b, t, n) x c, c a multiple of 16 up to 128, T <= 32, graphs zero-padded to Np = 16 ceil(N / 16) <= 448 (GPTST_ESHAPE beyond, nothing
 * written).  A block is BN_nodes(relu(step(relu(X)))).
 * step: with src = In (relu_in: relu(In)), per (b, tau) and node n
 *     Out[n, :] = cn oscale[n] (L (sscale . src))[n, :] + cw src[n, :] W + sum_k (ct M[tau][k] + [k = tau] cs) src[b, k, n, :]
 *   then relu (relu_out) and the mask [mask > 0] (mask NULL: none).  oscale, sscale (N) may be NULL (1); AT (rows, c; may be NULL) takes the
 *   bare node product L (sscale . src).  W (c, c), M (T, T) row-major.  In != Out.  Forward: L = A, oscale = sigmoid(alpha), M = W2^T,
 *   (cn, cw, ct, cs) = (3, 6, 6, -11); backward: L = A^T, sscale = sigmoid(alpha), W^T, M = W2, cs = -17, mask = the block's input.
 * wgrad: part (nsplit, c, c) = row-split partials of G^T relu(X); nsplit = gptst_stgode_wgrad_nsplit(rows, c); the caller sums the splits.
 * reduce: part2 (B * nparts, T, T) = partials of sum_{n, c} relu(X)[b, k, n, c] G[b, m, n, c], parta (B, N) = sum_{tau, c} G AT per (b, n);
 *   nparts = gptst_stgode_reduce_nparts(c, T, N); the caller sums over the first axis.
 * bn_stats: part (N, nsplit, 2) = (mean, sum of squared deviations from it) of each split of the B T rows of a node; nsplit =
 *   gptst_stgode_bn_nsplit(B T).  bn_apply: folds the splits (Chan, in double, index order) — part NULL: the running statistics instead —
 *   and writes Y = (Z - mean) rstd gamma + beta (Y may be NULL when best is given); training != 0 with part: rmean / rvar updated as torch
 *   does (momentum, unbiased variance); save_mean / save_rstd (N; may be NULL) for the backward.  best (rows, c; may be NULL): the running
 *   max over the branches — idx = 0 writes, a later idx replaces where strictly greater — and which (int32; may be NULL) the branch that holds it.
 * bn_bwd: dy = dY, or (dY NULL) dBest where which == idx.  stage 0: part (N, nsplit, 2) = split sums of dy and dy xhat; stage 1: G = [Z > 0]
 *   gamma rstd (dy - mean(dy) - xhat mean(dy xhat)) — the batch norm's backward and the mask of the step's relu — and dgamma, dbeta (N). */
int gptst_stgode_step(const float* L, int Np, const float* In, float* Out, float* AT, const float* W, const float* M, const float* oscale,
                      const float* sscale, const float* mask, float cn, float cw, float ct, float cs, int relu_in, int relu_out, int c, int B,
                      int T, int N, void* stream);
int gptst_stgode_wgrad_nsplit(int rows, int c);
int gptst_stgode_wgrad(const float* G, const float* X, int c, float* part, int nsplit, int rows, void* stream);
int gptst_stgode_reduce_nparts(int c, int T, int N);
int gptst_stgode_reduce(const float* G, const float* X, const float* AT, float* part2, float* parta, int c, int B, int T, int N, void* stream);
int gptst_stgode_bn_nsplit(int R);
int gptst_stgode_bn_stats(const float* Z, float* part, int nsplit, int c, int B, int T, int N, void* stream);
int gptst_stgode_bn_apply(const float* Z, const float* part, int nsplit, const float* gamma, const float* beta, float* rmean, float* rvar,
                          int training, float momentum, float eps, float* Y, float* save_mean, float* save_rstd, float* best, int* which, int idx,
                          int c, int B, int T, int N, void* stream);
int gptst_stgode_bn_bwd(const float* dY, const float* dBest, const int* which, int idx, const float* Z, const float* gamma, const float* mean,
                        const float* rstd, float* part, int nsplit, float* G, float* dgamma, float* dbeta, int c, int B, int T, int N, int stage,
                        void* stream);

int gptst_rowouter_ws_floats(int J, int C);   /* scratch (ws) size of gptst_rowouter */
/* first stage of gptst_rowouter alone: part (gptst_rowouter_nparts(rows), J*C + C + J) = row-chunk partials [sum a'^T X (j,c) | column
 * sums of X | sums of a'] for the caller to fold (one kind-1 pool job next to the other reductions of a step). */
int gptst_rowouter_nparts(int rows);
int gptst_rowouter_part(const float* a, int lda, const float* mask, float fill, const float* X, float* part, int want_asum, int rows,
                        int J, int C, void* stream);
int gptst_rowouter(const float* a, int lda, const float* mask, float fill, const float* X, float* out, int olayout, float* csum,
                   float* asum, float* ws, int rows, int J, int C, void* stream);

/* ---- time-index embeddings (timefeat.hip), GPTST.py:187-219 ------------------------------------------------
 * rows x K day/week features (K=1: time_feature, rows=B*T; K=12: time_feature_spg, rows=B) -> (rows, E).
 * The ten tensors are ln_day.{weight,bias}, ln_week.{..}, ln1.{..}, ln2.{..}, ln.{..}; bwd ACCUMULATES into g*. */
int gptst_timefeat_fwd(const float* wd, const float* bd, const float* ww, const float* bw, const float* w1, const float* b1,
                       const float* w2, const float* b2, const float* w3, const float* b3, const float* tidx, float* out, int rows,
                       int K, int E, void* stream);
int gptst_timefeat_bwd(const float* wd, const float* bd, const float* ww, const float* bw, const float* w1, const float* b1,
                       const float* w2, const float* b2, const float* w3, const float* b3, float* gwd, float* gbd, float* gww,
                       float* gbw, float* gw1, float* gb1, float* gw2, float* gb2, float* gw3, float* gb3, const float* tidx,
                       const float* dout, int rows, int K, int E, void* stream);

/* ---- fused thin heads (tails.hip): one pass over the C-wide activation where the loss meets the network --------------------
 * tail_mae: out = dec W^T + b (GPTST.py:455), masked-MAE statistics (Run.py:92-100, lib/metrics.py:11-18), gradient of the SUM loss
 *   w.r.t. dec -> d_dec (the 1/#kept of the mean is applied by gptst_clip_adam, hyper[9] = 1), per-workgroup partials
 *   part[blk][J*C + J] of (gW, gb) — gptst_tail_parts(rows) rows, summed by the caller (one kind-1 pool job) — and per-workgroup loss
 *   statistics sws[blk][4] = (sum |y-p|, kept count, -, -).
 * tail_kl: the backward through softmax + MLP_RL.ln3 (BasicTrainer.py:85, GPTST.py:33): d_h2, the partials of (gW3, gb3), and the
 *   KL sum of the workgroup in sws[blk][2].  prob (rows,HS) row-major, c (BT,HS,N).
 * stats_fold: stats[0..2] += the column sums of sws (rows, 4) in a fixed order (no float atomics anywhere on this path); rows the
 *   tail kernels did not write must be zero.  C = 64 and J / HS <= 16, else GPTST_ESHAPE (use the unfused ops).
 * premul != 0 (dPre chain, see gptst_hypertem_bwd): d_dec / d_h2 are multiplied by lrelu'(dec) / lrelu'(h2). */
int gptst_tail_parts(int rows);
int gptst_tail_mae(const float* dec, const float* W, const float* b, const float* src, int lda, const float* mask, float sigma, float mu,
                   float thresh, float* out, float* d_dec, float* part, float* sws, int premul, int rows, int J, int C, void* stream);
int gptst_tail_kl(const float* h2, const float* W3, const float* prob, const float* c, float w, float* d_h2, float* part, float* sws,
                  int premul, int rows, int N, int HS, int C, void* stream);
int gptst_stats_fold(const float* sws, int rows, float* stats, void* stream);

/* njobs (<= 16) time-feature instances in ONE launch (a step has seven).  params: njobs x 10 device pointers in the module order
 * above; grads likewise (bwd != 0 only, +=); io[q]: output (fwd) or output gradient (bwd) of job q; all jobs read one tidx. */
int gptst_timefeat_jobs(int njobs, int bwd, const void* const* params, const void* const* grads, const float* tidx,
                        const void* const* io, const int* rows, const int* K, const int* E, void* stream);
/* the backward (bwd = 1) carrying a table of npj gradient-reduction jobs (TAIL ROLES, at gptst_gram_bwd_jobs) */
int gptst_timefeat_jobs_bwd_jobs(int njobs, const void* const* params, const void* const* grads, const float* tidx, const void* const* io,
                                 const int* rows, const int* K, const int* E,
                                 int npj, const int* jkind, const void* const* jemb, const void* const* jx, const void* const* jpool,
                                 const void* const* jout, const int* jR, const int* jK, const int* jcols, const int* jnsplit, const int* jldx,
                                 void* stream);

/* start of a step in one launch (stepbegin.hip): zero z0[0..n0) (the [flat gradient | statistics] buffer: optimizer.zero_grad,
 * BasicTrainer.py:79) and z1[0..n1) (the step's zero-initialised scratch; may be NULL), and gather tidx (BT,2) = src[:, 0, base:base+2]
 * from src (BT, N, lda) (GPTST.py:256-257; tidx may be NULL); noise[0..n_noise) (may be NULL) <- the step's mask noise, uniform [0,1)
 * (torch.rand_like of GPTST.py:316,367,391) from Philox4x32-10 keyed by the DEVICE words rng[0] = seed, rng[1] = step counter. */
int gptst_step_begin(float* z0, long n0, float* z1, long n1, const float* src, float* tidx, int BT, int N, int lda, int base,
                     float* noise, long n_noise, const int* rng, void* stream);

/* ---- loss + optimiser (loss_adam.hip) ---------------------------------------------------------------------
 * stats: device float[8] zeroed once per step: [0] sum|y-p| [1] kept count [2] KL sum [3] extra sum g^2 terms (in; node-sharded
 * runs) [4] total sum g^2 (out) [6] [7] fold tickets of tails.hip.
 * mae: Run.py:92-100 + lib/metrics.py:11-18 + lib/normalization.py:23-27;  kl: Run.py:132 + BasicTrainer.py:85 (w = 0.1),
 * also emits the gradient w.r.t. the MLP_RL logits;  clip_adam: BasicTrainer.py:95-97 + Run.py:134 over flat buffers
 * (hyper layout documented in loss_adam.hip). */
int gptst_mae_fwd(const float* out, const float* src, int lda, const float* mask, float sigma, float mu, float thresh, int rows,
                  int J, float* stats, void* stream);
int gptst_mae_bwd(const float* out, const float* src, int lda, const float* mask, float sigma, float mu, float thresh, int rows,
                  int J, const float* stats, int normalize, float* dOut, void* stream);
int gptst_kl(const float* prob, const float* c, int rows, int N, int HS, float w, float* dlogit, float* stats, void* stream);
int gptst_clip_adam_ws_floats(void);   /* scratch floats (ws) of gptst_clip_adam: one gradient-norm partial per workgroup, folded in order */
int gptst_clip_adam(float* p, const float* g, float* m, float* v, long nA, long nB, const float* hyper, float* stats, float* ws,
                    float* stats_out, const float* sws, int sws_rows, void* stream);   /* stats_out (optional float[8]): copy of the final statistics block */

/* ---- layer-level entry points (layers.hip): ONE call per reference layer, forward and backward ---------------------------------------
 * SURVEY.md 8(b) "minimum set".  Host-side compositions of the kernel entry points above on the caller's stream; `saved` (forward ->
 * backward) and `scratch` (backward only) are caller-owned device regions of gptst_layer_bytes() bytes; no allocation / sync / host read.
 * Parameter and embedding gradients are ACCUMULATED (+=: zero them once), data gradients are written.  C = 64 and a (b,t) capsule matrix
 * that fits LDS (gptst_cap_fits_lds), else GPTST_ESHAPE; GPTST_EWS (-3) when a region is too small.
 * kind: 0 hyperTem (GPTST.py:154-163; uses d, Hm), 1 cap (:100-141; d, ds, HS, HT), 2 MLP_RL (:21-34; d, HS, base). */
int gptst_layer_bytes(int kind, int B, int T, int N, int C, int d, int Hm, int ds, int HS, int HT, int base, long* saved_bytes,
                      long* scratch_bytes);
/* hyperTem.forward(x, node_embeddings, time_eb) with parameters adj (d,Hm,T), weights_pool (d,C,C), bias_pool (d,C); time_eb (B*T,d). */
int gptst_hypertem_layer_fwd(const float* x, const float* node_emb, const float* time_eb, const float* adj, const float* wpool,
                             const float* bpool, float* out, void* saved, long saved_bytes, int B, int T, int N, int C, int d, int Hm,
                             void* stream);
int gptst_hypertem_layer_bwd(const float* dout, const float* x, const float* out, const float* node_emb, const float* time_eb,
                             const float* adj, const float* wpool, const float* bpool, const void* saved, long saved_bytes, float* dx,
                             float* d_node_emb, float* d_time_eb, float* d_adj, float* d_wpool, float* d_bpool, void* scratch,
                             long scratch_bytes, int B, int T, int N, int C, int d, int Hm, void* stream);
/* cap.forward(x, node_embeddings_spg, time_eb_spg (B,ds), teb (B*T,ds)) with ln_p, adj (ds,HS,N), t_adj (ds,HT,T*HS), weights_spa (d,C,C),
 * bias_spa (d,C), mask_template (T) -> out, c_out (B*T,HS,N) = the returned soft assignment, dyn_out (B,HT,T*HS); R = num_route. */
int gptst_cap_layer_fwd(const float* x, const float* node_emb_spg, const float* time_eb_spg, const float* teb, const float* ln_p_w,
                        const float* ln_p_b, const float* adj, const float* t_adj, const float* wspa, const float* bspa,
                        const float* mask_template, float* out, float* c_out, float* dyn_out, void* saved, long saved_bytes, int B, int T,
                        int N, int C, int d, int ds, int HS, int HT, int R, void* stream);
int gptst_cap_layer_bwd(const float* dout, const float* x, const float* out, const float* c, const float* dyn, const float* node_emb_spg,
                        const float* time_eb_spg, const float* teb, const float* ln_p_w, const float* ln_p_b, const float* adj,
                        const float* t_adj, const float* wspa, const float* bspa, const float* mask_template, const void* saved,
                        long saved_bytes, float* dx, float* d_node_emb_spg, float* d_time_eb_spg, float* d_teb, float* d_ln_p_w,
                        float* d_ln_p_b, float* d_adj, float* d_t_adj, float* d_wspa, float* d_bspa, void* scratch, long scratch_bytes, int B,
                        int T, int N, int C, int d, int ds, int HS, int HT, void* stream);
/* MLP_RL.forward(eb = a[:, :base] (rows = B*T*N, row stride lda), time_eb (B*T,d), node_eb (N,d)) -> logits (rows, HS); the input is data: no dx. */
int gptst_mlprl_layer_fwd(const float* a, int lda, const float* time_eb, const float* node_emb, const float* ln1_w, const float* ln1_b,
                          const float* wpool_spa, const float* bpool_spa, const float* wpool_tem, const float* bpool_tem, const float* ln3_w,
                          const float* ln3_b, float* logits, void* saved, long saved_bytes, int B, int T, int N, int C, int d, int base,
                          int HS, void* stream);
int gptst_mlprl_layer_bwd(const float* dlogits, const float* a, int lda, const float* time_eb, const float* node_emb, const float* ln1_w,
                          const float* wpool_spa, const float* bpool_spa, const float* wpool_tem, const float* bpool_tem, const float* ln3_w,
                          const void* saved, long saved_bytes, float* d_time_eb, float* d_node_emb, float* d_ln1_w, float* d_ln1_b,
                          float* d_wpool_spa, float* d_bpool_spa, float* d_wpool_tem, float* d_bpool_tem, float* d_ln3_w, float* d_ln3_b,
                          void* scratch, long scratch_bytes, int B, int T, int N, int C, int d, int base, int HS, void* stream);

/* ---- the downstream MSDR predictor's multi-state recurrence (msdr.hip; reference model/MSDR/gmsdr_cell.py:109-186, gpt-st_amd/predictors/msdr_hip.py) ---
 * A cell keeps its last Kk outputs.  Per step t, with h the newest: pre = Gx_t + [h, L_1 h, .., A h] Th, c = leaky_relu(pre), a = softmax_k(w .
 * vec(s_k + R_k) + bias), o = c W + b + sum_k a_k (s_k + R_k).  Gx and every weight / graph / input gradient are hoisted onto gptst_stgcn_nodemix /
 * tapgemm / wgrad and gptst_mtgnn_graphgrad; these launches are the state chain.  All rows are TIME-major: row (t B + b) N + n of a "seq" tensor
 * (T B N, width).  Hs (T + Kk, B N, Hp) is the state ring: slots [0, Kk) the initial states, oldest first, slot Kk + t the output of step t; dH
 * is its gradient, same shape.  Hp = rnn_units zero-padded to a multiple of 16 (16 .. 128); 1 <= Kk <= 8; L (ks, Np, Np) zero-padded to Np = 16
 * ceil(N / 16), ks = 2 or 3: the fixed supports, then A.  G = gptst_msdr_groups(N, B, tiles) workgroups serve a sample (tiles: 0 = the kernel's
 * choice, 1 or 2 row tiles of 16 nodes per workgroup); partial rows have G entries and are folded in index order (no atomics).
 * fwd_step: Wh (Hp, (ks + 1) Hp) = the state rows of Theta, column m Hp + i = (matrix m, input channel i), matrix 0 the identity;  W2 (Hp, Hp) =
 *   W^T;  bvec, w, w2 (N, Hp);  R (Kk, N, Hp);  wr (Kk) = w . R_k + bias;  Gx (seq, Hp).  Reads slots t .. t + Kk - 1 of Hs and of sig (T + Kk,
 *   B, G: the partials of w . s), writes slot t + Kk of both — and of sig2 with w2 (both or neither).  Kept when not NULL: c (seq, Hp), z (seq,
 *   ldz = (ks + 1) Hp) = [h | L_k h]_k, a (T, B, Kk).
 * bwd_pre: W (Hp, Hp);  dO = slot Kk + t of dH  ->  dpre (seq, Hp)[t] = (dO W^T) leaky'(c), pa (B, G, 8)[.., k] = partial of <dO, s_k + R_k>.
 * bwd_state: LT (ks, Np, Np) the transposes;  WhT (Hp, (ks + 1) Hp), column m Hp + j = Theta_m[i][j];  de (T, B, Kk)[t] = a (dA - sum a dA);
 *   slots t + k of dH += a_k dO + de_k w, slot t + Kk - 1 also += [dpre | L_k^T dpre]_k WhT^T.
 * lds_bytes: the dynamic LDS of the widest of the three at this shape (above 160 KB they return GPTST_ESHAPE). */
int gptst_msdr_lds_bytes(int N, int Hp, int B, int ks);
int gptst_msdr_groups(int N, int B, int tiles);
int gptst_msdr_fwd_step(const float* L, int Np, int ks, const float* Wh, const float* W2, const float* bvec, const float* R, const float* w,
                        const float* w2, const float* wr, const float* Gx, float* Hs, float* sig, float* sig2, float* c, float* z, int ldz,
                        float* a, int B, int T, int N, int Hp, int Kk, int t, int tiles, void* stream);
int gptst_msdr_bwd_pre(const float* W, const float* R, const float* Hs, const float* dH, const float* c, float* dpre, float* pa, int B, int T,
                       int N, int Hp, int Kk, int t, int tiles, void* stream);
int gptst_msdr_bwd_state(const float* LT, int Np, int ks, const float* WhT, const float* w, const float* a, const float* pa, const float* dpre,
                         float* dH, float* de, int B, int T, int N, int Hp, int Kk, int t, int tiles, void* stream);

/* ---- the downstream ST-WA predictor's cuts (stwa.hip; reference model/ST_WA/ST_WA.py:138-164, attention.py, gpt-st_amd/predictors/stwa_hip.py) ----
 * C = 16 or 32 channels, 8 heads of C / 8.  A Layer has `cuts` sequential cuts of `cs` <= 6 data rows; cut i reads R = clamp(T - i cs, 0, cs) rows of
 * h (B, T, N, C) from row i cs, the proxies prox (2 cuts, N, C)[2 i, 2 i + 1] and out_{i-1} = slot i - 1 of Y (B, cuts, N, C) (cut 0: nothing).
 * The four generated maps (0 temporal key, 1 temporal value, 2 spatial key, 3 spatial value) come factored: V (4, 6, C, C) with x V[g][k] = sum_i
 * x_i V[g][k][i][.], u (4, 6, C), and the per-(sample, node) coefficients co, cb (B, N, 4, 5) of entries 1 .. 5 (entry 0 has coefficient 1).  The six
 * shared Linears (temporal projection1, projection2, spatial projection1, projection2, aggregator 0, 2) are Wl (6, C, C) [out][in], WlT their
 * transposes, bl (6, C).  Tq, Ks, Vs, S, dS, dTq, dKs, dVs are (B, 2, N, C); mx, sm, Dq (B, 2, N, 8).
 * local_fwd: -> Tq (the temporal attention's output), Ks, Vs.   spatial_fwd: -> slot `cut` of Y; S, mx, sm are written when not NULL (mx, sm: both
 *   or neither).   spatial_bwd_q: dY (B, cuts, N, C) slot `cut` + carry (B, N, C; NULL: none) -> dS, Dq, dTq.   spatial_bwd_kv: -> dKs, dVs.
 * local_bwd: -> rows [cut cs, cut cs + R) of dh (B, T, N, C), slots 2 cut, 2 cut + 1 of dPb (B, 2 cuts, N, C) (the proxies' gradient per sample) and
 *   carry = the gradient of out_{cut-1} — each written when not NULL — and ADDS to dco, dcb (B, N, 4, 5).
 * slab (NULL: no weight gradient is computed): (B ceil(N / 16), gptst_stwa_slab_floats(C)), one row per workgroup, ADDED to by spatial_bwd_q and
 *   local_bwd: [dV (4, 6, C, C) | du (4, 6, C) | dWl (6, C, C) | dbl (6, C)]; the caller zeroes it and sums its rows.  du of map 0 stays 0 (a bias
 *   common to all keys of a softmax), and so does its share of dcb.
 * lds_bytes: the dynamic LDS of the widest of the five launches at this shape (above 160 KB they return GPTST_ESHAPE). */
int gptst_stwa_lds_bytes(int N, int C);
int gptst_stwa_slab_floats(int C);
int gptst_stwa_local_fwd(const float* h, const float* prox, const float* Y, const float* co, const float* cb, const float* V, const float* u,
                         const float* WlT, const float* bl, float* Tq, float* Ks, float* Vs, int B, int T, int N, int C, int cuts, int cut, int cs,
                         void* stream);
int gptst_stwa_spatial_fwd(const float* Tq, const float* Ks, const float* Vs, const float* WlT, const float* bl, float* Y, float* S, float* mx,
                           float* sm, int B, int N, int C, int cuts, int cut, void* stream);
int gptst_stwa_spatial_bwd_q(const float* Tq, const float* Ks, const float* Vs, const float* S, const float* mx, const float* sm, const float* Wl,
                             const float* WlT, const float* bl, const float* dY, const float* carry, float* dS, float* Dq, float* dTq, float* slab,
                             int B, int N, int C, int cuts, int cut, void* stream);
int gptst_stwa_spatial_bwd_kv(const float* Tq, const float* Ks, const float* Vs, const float* dS, const float* Dq, const float* mx, const float* sm,
                              float* dKs, float* dVs, int B, int N, int C, void* stream);
int gptst_stwa_local_bwd(const float* h, const float* prox, const float* Y, const float* co, const float* cb, const float* V, const float* u,
                         const float* Wl, const float* WlT, const float* bl, const float* dTq, const float* dKs, const float* dVs, float* dh,
                         float* dPb, float* carry, float* dco, float* dcb, float* slab, int B, int T, int N, int C, int cuts, int cut, int cs,
                         void* stream);

/* ---- the downstream ST-MGCN predictor's stacked LSTM (stmgcn.hip; reference model/STMGCN_demand/STMGCN.py:19-20,45-48, gpt-st_amd/predictors/stmgcn_hip.py) ---
 * L <= 4 layers of width H (a multiple of 16 up to 128) over `rows` independent rows and T <= 32 steps, zero initial state, gate blocks in torch's
 * order i, f, g, o.  All tensors are TIME-major.  The input half of layer 0 is hoisted: Gx0 (T, rows, 4H) = x_t W_ih0^T + b_ih0 + b_hh0.
 * W: W_hh0 (4H, H) followed by [W_ih_l | W_hh_l] (4H, 2H) for l = 1 .. L-1;  WT: the transposes (H, 4H), (2H, 4H) in the same order;  bias (L, 4H) =
 * b_ih_l + b_hh_l (row 0 is not read).
 * lstm_fwd: ONE launch.  Either top (T, rows, H) = the top layer's h of every step and nothing else (gates = c = h = NULL), or — for a backward —
 *   gates (L, T, rows, 4H) activated, c (L, T, rows, H) and h (L, T + 1, rows, H) whose slot 0 the caller has zeroed (top = NULL: it is h[L-1][1:]).
 * lstm_bwd: ONE launch.  dTop (T, rows, H) = the gradient of every step of the top ring -> dG (dG_layers, T, rows, 4H), the gradient of the
 *   pre-activations of layers 0 .. dG_layers - 1 (dG[0] is dGx0; 1 <= dG_layers <= L: layers above are computed and not stored).  The weight
 *   gradients are gptst_stgcn_wgrad of dG against slices of h.
 * A workgroup owns `tiles` 16-row tiles (0: gptst_stmgcn_tiles' choice, the same in both launches); lds_bytes: the larger dynamic LDS of the two
 * launches at (H, L, tiles); above 160 KB they return GPTST_ESHAPE. */
int gptst_stmgcn_lds_bytes(int H, int L, int tiles);
int gptst_stmgcn_tiles(int rows, int H, int L, int forced);
int gptst_stmgcn_lstm_fwd(const float* Gx0, const float* W, const float* bias, float* top, float* gates, float* c, float* h, int rows, int T, int L,
                          int H, int tiles, void* stream);
int gptst_stmgcn_lstm_bwd(const float* dTop, const float* WT, const float* gates, const float* c, float* dG, int dG_layers, int rows, int T, int L,
                          int H, int tiles, void* stream);

/* ---- the downstream CCRNN predictor's graph-GRU cell (ccrnn.hip; reference model/CCRNN_demand/CCRNN.py:39-60,198-233, gpt-st_amd/predictors/ccrnn_hip.py) ---
 * One cell step at one graph-conv layer on one support: P (ks, Np, Np) = [T_1(S) .. T_ks(S)] zero-padded (PT: their transposes), ks <= 3; the
 * operand slab of sample b is [state part (Hp) | input part (Cp)], Hp in {16, 32}, Cp a multiple of 16, Hp + Cp <= 64; M = [slab | P_j slab]_j.
 * Step tensors are (B*N, width) with row b N + n, seq tensors (B*T*N, width) with row (b T + t) N + n.  Weights are matrix-major:
 *   W0 (2 Hp, (ks + 1)(Hp + Cp)) rows [r | u], W1 (Hp, (ks + 1)(Hp + Cp));  W1T (Hp + Cp, (ks + 1) Hp), W0T (Hp + Cp, (ks + 1) 2 Hp): rows [dstate | dinput].
 * fwd_gates: [r, u] = sigmoid(M([h | inp]) W0^T + g) -> u, q = r h, and when given r and z (seq, (ks + 1)(Hp + Cp)) = M.  g: exactly one of Gx0
 *   (seq, 2 Hp: the hoisted input half with the bias, Cp = 0) and bias (2 Hp).  With Cp > 0 exactly one of inp (B*N, Cp) and fb_h: then the
 *   input is fb_h fb_W^T + fb_b (fb_h (B*N, Hp), fb_W (Cp, Hp), fb_b (Cp)) formed on load and stored in inp_out (B*N, Cp).
 * fwd_state: c = tanh(M([q | inp]) W1^T + g) -> h_out = u h + (1 - u) c, and when given c and z.
 * bwd_cand: dpre1[:, t] = (dh + dh2)(1 - u)(1 - c^2) (dh2 may be NULL);  [dq | dinp] = M^T-side product with W1T;  dpre0[:, t] = [dq h r (1 - r) |
 *   (dh + dh2)(h - c) u (1 - u)];  dh_part = (dh + dh2) u + dq r;  dinp (B*N, Cp) = the candidate's share.
 * bwd_state: dh_out = dh_part + dstate(dpre0[:, t]);  dinp += dinput(dpre0[:, t]).
 * lds_bytes: the largest dynamic LDS of the four launches; above 160 KB they return GPTST_ESHAPE.  tiles as in gptst_tgcn_*. */
int gptst_ccrnn_lds_bytes(int N, int Hp, int Cp, int ks, int B);
int gptst_ccrnn_fwd_gates(const float* P, int Np, int ks, const float* W0, const float* h, const float* inp, int Cp, const float* fb_h,
                          const float* fb_W, const float* fb_b, float* inp_out, const float* Gx0, const float* bias, float* u, float* r,
                          float* q, float* z, int B, int T, int N, int Hp, int t, int tiles, void* stream);
int gptst_ccrnn_fwd_state(const float* P, int Np, int ks, const float* W1, const float* q, const float* inp, int Cp, const float* Gx1,
                          const float* bias, const float* u, const float* h, float* h_out, float* c, float* z, int B, int T, int N,
                          int Hp, int t, int tiles, void* stream);
int gptst_ccrnn_bwd_cand(const float* PT, int Np, int ks, const float* W1T, int Cp, const float* dh, const float* dh2, const float* u,
                         const float* c, const float* r, const float* h, float* dpre1, float* dpre0, float* dh_part, float* dinp, int B,
                         int T, int N, int Hp, int t, int tiles, void* stream);
int gptst_ccrnn_bwd_state(const float* PT, int Np, int ks, const float* W0T, int Cp, const float* dpre0, const float* dh_part,
                          float* dh_out, float* dinp, int B, int T, int N, int Hp, int t, int tiles, void* stream);

/* ---- the downstream DMVSTNET predictor's semantic view (dmvstnet.hip; reference model/DMVSTNET_demand/DMVSTNET.py:57-61, gpt-st_amd/predictors/dmvstnet_hip.py) ---
 * z[r, :] = x[r, :] V[n] + c[n], n = r mod N; x (units, N, C), V (N, C, O), c (N, O), C a multiple of 16 up to 128, 1 <= O <= 4, else GPTST_ESHAPE.
 * sen_fwd: z (units, N, O).   sen_bwd: dx (units, N, C) = dz V[n]^T, and pV (nsplit, N, C, O), pc (nsplit, N, O) = unit-split partials of
 *   dV[n] = sum_units x^T dz and dc[n] = sum_units dz, each over its units in ascending order; nsplit = gptst_dmvst_sen_nsplit(units, N) (else
 *   GPTST_EARG); the caller sums the splits (fixed order, no atomics). */
int gptst_dmvst_sen_nsplit(int units, int N);
int gptst_dmvst_sen_fwd(const float* x, const float* V, const float* c, float* z, int units, int N, int C, int O, void* stream);
int gptst_dmvst_sen_bwd(const float* x, const float* V, const float* dz, float* dx, float* pV, float* pc, int nsplit, int units, int N, int C, int O,
                        void* stream);

/* ---- communication (comm.hip): RCCL over xGMI with an explicit stream — a collective can sit inside a captured hipGraph -------------
 * The reference has no distributed code; these carry the data-parallel gradient exchange (one all-reduce of [flat gradient | statistics])
 * and the node-sharded cluster aggregations.  RCCL is bound at run time (dlopen): -4 (GPTST_ECOMM) when it is not available or no
 * communicator is given, 1000 + ncclResult_t on an RCCL error.  Communicators are HANDLES (r04; a process-global one before): a process may
 * hold several — the row and the column of a data-parallel x node-shard mesh (SURVEY 8(e) "Combination") — each created by gptst_comm_init
 * on the ranks that form it.  unique_id: 128 bytes (ncclUniqueId) created on one rank of the communicator and distributed by the caller. */
int gptst_comm_available(void);                                /* RCCL can be bound here (no bootstrap, no socket): the probe before a communicator is formed */
int gptst_comm_unique_id(void* out128);
int gptst_comm_init(int rank, int world, const void* unique_id, void** comm_out);    /* *comm_out: the handle the calls below take */
int gptst_allreduce_f32(void* comm, float* buf, long n, void* stream);      /* in-place sum over the ranks */
/* recv[r*n .. (r+1)*n) <- rank r's send[0..n), 32-bit words (the cluster labels of a data-parallel global batch); send may be recv + rank*n */
int gptst_allgather_i32(void* comm, const int* send, int* recv, long n, void* stream);
int gptst_comm_count(void* comm, int* out);                    /* ncclCommCount of the communicator */
int gptst_comm_destroy(void* comm);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* GPTST_HIP_H */
