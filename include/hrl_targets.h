/*
 * hrl_targets.h — C ABI of the MI355X return-target scans (libhrl.so).
 *
 * Replaces the reference operator
 *     handyrl.losses.compute_target(algorithm, values, returns, rewards,
 *                                   lmb, gamma, rhos, cs)
 * (reference: handyrl/losses.py:61-74, with the recurrences at
 *  losses.py:16-17 monte_carlo, :20-28 temporal_difference, :31-40 upgo,
 *  :43-58 vtrace) and its two/four call sites in compute_loss
 * (handyrl/train.py:245-253).
 *
 * Conventions (all pointers are DEVICE pointers, fp32; C-contiguous for
 * hrl_compute_target and hrl_compute_targets_fused, any non-negative strides
 * for hrl_compute_targets_strided, see there):
 *   values   (B, T, C)       C = P*K value columns (P players x K value dims)
 *   returns  (B, ret_T, C)   ret_T in {1, T}; TD/UPGO/VTRACE read only the
 *                            last time step (the bootstrap), MC reads all
 *   rewards  (B, T, C)       may be NULL  (reference: rewards=None -> 0)
 *   rhos, cs (B, T, rho_C)   rho_C in {1, P}; value column c reads rho column
 *                            c / rho_div  (rho_div = K when rho_C == P,
 *                            rho_div = C when rho_C == 1: broadcast)
 *   lmb, gamma               passed as double; the kernels use the same float
 *                            coefficients the reference's Python-scalar x
 *                            float32-tensor arithmetic uses: (float)(1-lmb),
 *                            (float)lmb, (float)gamma, (float)(gamma*lmb)
 * Outputs (caller-allocated, (B, T, C)):
 *   targets  may be NULL (MC's target is `returns` itself, losses.py:17)
 *   advantages
 *
 * Every entry point is asynchronous on `stream` (a hipStream_t; pass torch's
 * current stream), allocates nothing, never synchronises and reads nothing
 * back to the host, so it may be captured into a hipGraph.
 * Return value: 0 on success, HRL_EINVAL for a bad algorithm / shape /
 * pointer, HRL_ELAUNCH_BASE - hipError_t for a launch failure.
 */
#ifndef HRL_TARGETS_H
#define HRL_TARGETS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    HRL_ALG_MC = 0,      /* losses.py:16  */
    HRL_ALG_TD = 1,      /* losses.py:20  */
    HRL_ALG_UPGO = 2,    /* losses.py:31  */
    HRL_ALG_VTRACE = 3,  /* losses.py:43  */
};

#define HRL_OK 0
#define HRL_EINVAL (-22)
#define HRL_ELAUNCH_BASE (-1000)

/* ABI version, bumped on any signature change. */
int hrl_abi_version(void);

/* Human-readable text for a return code (static storage). */
const char *hrl_strerror(int code);

/* Kernel form of the scans for T <= 16: 2 one lane per (trajectory, column) straight from global memory (no
 * LDS), 0 the chunked LDS-transpose kernel every T uses, 1 (the default) the first for small batches
 * (B*C <= 32768) and the second otherwise.  Results are bit-identical.  Process-wide; returns the previous
 * setting. */
int hrl_targets_set_short_form(int form);

/*
 * One algorithm, one head: the drop-in for a single compute_target call
 * (losses.py:61).  targets may be NULL; for MC it must be NULL.
 */
int hrl_compute_target(int alg,
                       const float *values, const float *returns, const float *rewards,
                       const float *rhos, const float *cs,
                       int64_t B, int64_t T, int64_t C, int64_t ret_T,
                       int64_t rho_C, int64_t rho_div,
                       double lmb, double gamma,
                       float *targets, float *advantages,
                       void *stream);

/*
 * Fused learner form of train.py:248-253 for one head: ONE pass over the
 * inputs produces the value-target of `target_alg` (args['value_target'])
 * and the advantages of `adv_alg` (args['policy_target']; the reference
 * discards value_target's advantages when the two differ, train.py:251-253).
 * targets may be NULL (and must be for target_alg == MC).
 */
int hrl_compute_targets_fused(int target_alg, int adv_alg,
                              const float *values, const float *returns, const float *rewards,
                              const float *rhos, const float *cs,
                              int64_t B, int64_t T, int64_t C, int64_t ret_T,
                              int64_t rho_C, int64_t rho_div,
                              double lmb, double gamma,
                              float *targets, float *advantages,
                              void *stream);

/*
 * The fused form for operands that are VIEWS: a time window of a longer
 * buffer, a time-major buffer seen as (B, T, ...), a column slice, an outcome
 * expanded over value dimensions.  Nothing is copied or allocated.
 *
 * Every operand has the logical shape (B, T, P, K) (returns: (B, ret_T, P, K))
 * with C = P*K <= 64 value columns, and is addressed as
 *     base[b*sB + t*sT + p*sP + k*sK]
 * strides: HOST array of 5 x 4 int64 ELEMENT strides (sB, sT, sP, sK) for
 *   values, returns, rewards, rhos, cs, in that order; read before the call
 *   returns.  A stride of 0 broadcasts along that axis; the stride of an axis
 *   of extent 1 is ignored, as is the whole row of a NULL operand.  Strides
 *   are non-negative.
 * The strides alone say how rhos / cs broadcast (this replaces rho_C and
 * rho_div), and rhos and cs may differ: (B,T,1,1), (B,T,P,1), (B,T,1,K),
 * (B,1,P,1) over time, ... all pass as stride-0 axes.
 * target_alg == adv_alg gives the single-algorithm form of hrl_compute_target.
 * Outputs are C-contiguous (B, T, P, K) and MUST NOT alias any input (an
 * input element may be read after the output element of another trajectory
 * has been written).
 *
 * Addressing: the trajectory term b*sB is applied in 64-bit arithmetic, so
 * sB may be of any size; the kernels add the inner term t*sT + p*sP + k*sK
 * as a 32-bit integer, so a call whose largest inner offset
 *     (T-1)*sT + (P-1)*sP + (K-1)*sK
 * (ret_T-1 for returns) reaches 2^31 elements, or whose largest offset
 * reaches 2^60 elements, is rejected with HRL_EINVAL.
 *
 * HRL_EINVAL, before any HIP call, for: NULL strides; a negative stride;
 * P < 1, K < 1 or P*K > 64; and what the entry points above reject (unknown
 * algorithm, T < 1, ret_T not in {1, T}, MC with targets, V-trace without
 * rhos / cs, a NULL values / returns / advantages).  B == 0 returns HRL_OK
 * and touches nothing.
 * A call whose operands are all C-contiguous, with rhos and cs both
 * (B,T,1,1), both (B,T,P,1) or both (B,T,P,K), launches the same kernel as
 * hrl_compute_targets_fused.
 */
int hrl_compute_targets_strided(int target_alg, int adv_alg,
                                const float *values, const float *returns, const float *rewards,
                                const float *rhos, const float *cs, const int64_t *strides,
                                int64_t B, int64_t T, int64_t P, int64_t K, int64_t ret_T,
                                double lmb, double gamma,
                                float *targets, float *advantages,
                                void *stream);

#ifdef __cplusplus
}
#endif

#endif /* HRL_TARGETS_H */
