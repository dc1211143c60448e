// cms.h -- one totally skewed alpha/2-stable draw by Chambers-Mallows-Stuck in fp64, keyed by a Philox counter: the heavy-tailed a
// of the held-out losses (loss.hip, lim_loss.hip), evaluated exactly as noise.hip's k_skewed_levy evaluates it (S1, beta = 1,
// stability alpha/2, scale 2 cos(pi alpha / 4)^(2 / alpha)).
#pragma once
#include "philox.h"

namespace dlpm {

struct Cms {
    double a, zeta, th0, scale;
};

__device__ inline Cms cms_setup(double alpha) {
    const double pi = 3.141592653589793;
    Cms c;
    c.a = alpha * 0.5;
    c.zeta = tan(pi * c.a * 0.5);
    c.th0 = atan(c.zeta) / c.a;
    c.scale = 2.0 * pow(cos(pi * alpha * 0.25), 2.0 / alpha);
    return c;
}

__device__ inline float cms_draw(const Cms &c, uint64_t seed, uint64_t gidx, uint32_t row, uint32_t purpose, uint32_t rep) {
    const double pi = 3.141592653589793;
    uint4 r = philox4x32_10(make_uint4((uint32_t)gidx, (uint32_t)(gidx >> 32), row, purpose | (rep << 8)), seed);
    double U = ((double)(((uint64_t)r.x << 21) ^ (r.y >> 11)) + 0.5) * (1.0 / 9007199254740992.0);
    double V = ((double)(((uint64_t)r.z << 21) ^ (r.w >> 11)) + 0.5) * (1.0 / 9007199254740992.0);
    double W = -log(V);
    double th = U * pi + (-pi / 2.0);
    double ath = c.a * th, cs = cos(th), tg = tan(th);
    double lead = W / (cs / tan(c.a * (c.th0 + th)) + sin(th));
    double core = (cos(ath) + sin(ath) * tg - c.zeta * (sin(ath) - cos(ath) * tg)) / W;
    return (float)(lead * pow(core, 1.0 / c.a) * c.scale);
}

}  // namespace dlpm
