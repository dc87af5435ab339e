// invconv_lu.h -- launcher interface of invconv_lu.hip: the LU-parameterised invertible 1x1 convolution
//   W = P (tril(l, -1) + I) (triu(u, 1) + diag(sign_s exp(log_s)))
// (the form the Glow paper trains; the reference stops at network/module.py:336-337).  No factorisation anywhere: W is a
// triangular product, log|det W| = sum(log_s), W^-1 two substitutions per column, the gradients two triangular products.
#pragma once
#include "common.h"

namespace glowhip {

constexpr int INVCONV_LU_MAX_C = 512;   // the inverse kernel keeps 16 solution columns (fp64) and a 16-row panel in LDS

// One LU-form layer of a pack.  perm: row table of P (row i of P has its one in column perm[i], so W[i] = (L U_f)[perm[i]]).
// Entries of l on or above the diagonal and of u on or below it are never read.
struct LuJob {
    const int32_t* perm; const float* l; const float* u; const float* log_s; const float* sign_s;
    float* w;                  // out: the assembled matrix (C, C)
    const float* an_logs;      // plan: actnorm.logs of the step (its term of the constant); null: stand-alone call
    int C, HW;
    size_t winv_off, logabsdet_off, konst_off;   // plan: byte offsets into `packed`, filled as k_step_prepare_* fills them
    float* winv; float* logabsdet;               // stand-alone call (packed == null): outputs, either may be null
};
// jobs_dev: n jobs in device memory, or null with n == 1 and `single` passed by value (the stand-alone entry points)
int launch_invconv_lu_assemble(const LuJob* jobs_dev, const LuJob* single, int n, int max_c, void* packed, hipStream_t s);
int launch_invconv_lu_inverse(const LuJob* jobs_dev, const LuJob* single, int n, int max_c, void* packed, hipStream_t s);

// dl = strict-lower(P^T G U_f^T), du = strict-upper(L^T P^T G), dlog_s[i] = (L^T P^T G)[i][i] sign_s[i] exp(log_s[i]) + term,
// term = (gsum ? gsum[0] : 1) * term_mul; G = dw, the gradient w.r.t. the assembled matrix without any log-det part.
// Every masked entry of dl / du is written as 0.
struct LuGradJob {
    const int32_t* perm; const float* l; const float* u; const float* log_s; const float* sign_s;
    const float* dw; float* dl; float* du; float* dlog_s;
    int C;
    const double* gsum; double term_mul;
};
int launch_invconv_lu_backward(const LuGradJob* jobs_dev, const LuGradJob* single, int n, int max_c, hipStream_t s);

}  // namespace glowhip
