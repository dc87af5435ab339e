// tophead.h -- the "top head" of Glow: learned / class-conditional top prior + classifier (tophead.hip).
#pragma once
#include "common.h"
#include "sampler_rng.h"

struct glowhip_plan;

namespace glowhip {

// floats of per-sample head state kept between the training forward and its backward: [mean | logs] (2C), e = y_emb(y_onehot)
// (2C), h_y = mean_{H,W} z (C)
static inline size_t head_state_floats(int N, int C) { return (size_t)N * 5 * C; }

// The top prior's log-density of z into acc: the head's one launch when a head is attached to the plan, k_gaussian_logp otherwise.
int launch_top_logp(glowhip_plan* plan, const float* z, const float* prior_mean, const float* prior_logs, long prior_stride,
                    int N, unsigned long long* acc, hipStream_t s);
// The top latent of a sampler call in one launch: z = mean + exp(logs) * draw with (mean, logs) the plan's prior (zeros, or the
// attached head's learn_top / y_emb(y_onehot) rows, plus the optional dense base) and draw = stream 0 of `rng` (sampler_rng.h).
// No dense mean / logs in HBM.
int launch_top_sample(glowhip_plan* plan, const float* prior_mean, const float* prior_logs, long prior_stride, const SamplerSpec& rng,
                      float* z, int N, hipStream_t s);
// dL/dz at the top (+ the head's parameter gradients when a head is attached): k_top_head_bwd (+ k_top_head_reduce) or k_prior_bwd.
// gh: N * 2C floats of scratch (only read / written when a head is attached).
int launch_top_bwd(glowhip_plan* plan, const float* z, const float* prior_mean, const float* prior_logs, long prior_stride,
                   const float* gld, const float* z_grad, float* gz, float* gh, int N, hipStream_t s);

}  // namespace glowhip
