// Denoising loss terms on the device (losses.hip): the eval-mode forward of the reference's training objective.
#pragma once
#include "dsh_common.h"

namespace dsh {

// result_dev layout, argument rules and the terms themselves: include/diffsheg_hip.h (dsh_op_denoise_losses)
long long denoise_losses_result_bytes(int B, int T);
int launch_denoise_losses(const float* eps, const float* noise, const float* x_t, const float* x0, const float* c1_dev, const float* c2_dev,
                          const int* lens_dev, int B, int T, int C, int split, float huber_beta, float* x0_pred_out, float* frame_mse_out,
                          void* result_dev, hipStream_t s);

}  // namespace dsh
