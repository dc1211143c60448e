// conv_splitk.hip -- a split-K convolution launch (launch_conv_splitk) and the reduction behind it (round 6).
//
// At a small DECLARED batch the 8x8 / 4x4 levels of a UNet launch 16-128 workgroups that each walk a K loop of 32-64 serial phases
// (the CIFAR net at B = 64: 14 F(2x2) launches of ~100 us on 16 workgroups).  conv_route (ConvRoute::ksplit) cuts that loop over 2 / 4 / 8 grid copies
// (ConvLaunch::ksplit: the narrow F(4x4) shapes and the F(2x2) kernel); copy s leaves the partial OUTPUTS of its channel range -- the
// Winograd output transform is linear, so partial sums may be transformed before they are added -- in part[s], and this kernel forms
//     out = bias + (((part[0] + part[1]) + part[2]) + ...) (+ residual)
// in a fixed order: deterministic, a function of the layer and the declared batch only.  Replaces nothing in the reference (the
// convolution is F.conv2d, dlpm/models/unet.py:143,157 via nn.py:25-35); it is the tail of those launches.
#include "conv.h"

namespace dlpm {
namespace {

__global__ void __launch_bounds__(256) k_splitk_reduce(const float *__restrict__ part, int S, int64_t n4, int64_t stride4, int Cout,
                                                       const float *__restrict__ bias, const float *__restrict__ res0,
                                                       const float *__restrict__ res1, int R0, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 *p4 = reinterpret_cast<const float4 *>(part);
    float4 a = p4[i];
    for (int s = 1; s < S; s++) {
        const float4 b = p4[i + (int64_t)s * stride4];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    const int c4 = Cout >> 2;
    const int64_t pix = i / c4;
    const int c = (int)(i - pix * c4) * 4;
    if (bias) {
        const float4 b = *reinterpret_cast<const float4 *>(bias + c);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    if (res0) {
        const float4 r = c < R0 ? *reinterpret_cast<const float4 *>(res0 + pix * R0 + c)
                                : *reinterpret_cast<const float4 *>(res1 + pix * (Cout - R0) + (c - R0));
        a.x += r.x; a.y += r.y; a.z += r.z; a.w += r.w;
    }
    reinterpret_cast<float4 *>(out)[i] = a;
}

}  // namespace

int launch_splitk_reduce(const float *part, int S, int64_t npix, int Cout, const float *bias, const float *res0, const float *res1, int R0,
                         float *out, hipStream_t st) {
    DLPM_CHECK_ARG(part && out && S >= 2 && npix > 0 && (Cout & 3) == 0 && (R0 & 3) == 0, "launch_splitk_reduce: bad argument");
    const int64_t n4 = npix * (Cout >> 2);
    ProfScope ps("splitk_reduce", 0.0, 4.0 * (double)npix * Cout * (S + 1 + (res0 ? 1 : 0)), st);
    k_splitk_reduce<<<(unsigned)ceil_div(n4, 256), 256, 0, st>>>(part, S, n4, n4, Cout, bias, res0, res1, R0 ? R0 : Cout, out);
    DLPM_LAUNCH_CHECK();
    return DLPM_OK;
}

int64_t splitk_partial_floats(const ConvLaunch &c, const ConvRoute &r) {
    return r.ksplit > 1 ? (int64_t)r.ksplit * c.B * c.Hout * c.Wout * c.Cout : 0;
}

// The ONE definition of a split-K launch: the plan (unet.hip: run_conv3) and the kernel-level entry (dlpm_conv_policy_f32) both run this.
int launch_conv_splitk(const ConvLaunch &c, const ConvRoute &r, float *part, hipStream_t st) {
    const int S = r.ksplit;
    if (S <= 1) return launch_conv(c, nullptr, nullptr, st);
    DLPM_CHECK_ARG(part, "launch_conv_splitk: a split-K launch needs its partial buffer");
    ConvLaunch P = c;
    P.bias = nullptr; P.res0 = nullptr; P.res1 = nullptr; P.R0 = 0; P.stats_out = nullptr; P.out = part; P.ksplit = S;
    const int rc = launch_conv(P, nullptr, nullptr, st);
    if (rc != DLPM_OK) return rc;
    return launch_splitk_reduce(part, S, (int64_t)c.B * c.Hout * c.Wout, c.Cout, c.bias, c.res0, c.res1, c.R0, c.out, st);
}

}  // namespace dlpm
