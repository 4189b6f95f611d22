// cubic.h -- the cubic convolution weights of the x2 bicubic up-sampling (torch.nn.functional.interpolate: A = -0.75), shared by the forward
// (encoder_ops.hip) and its transpose (resample_bwd.hip) so that both evaluate the same fp32 expression.
#pragma once

// w[i] = the weight of tap floor(f) - 1 + i for the fractional part t = f - floor(f)
__device__ __forceinline__ void cubic_w(float t, float *w)
{
    const float A = -0.75f;
    const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
    w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
    w[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
    w[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
    w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}
