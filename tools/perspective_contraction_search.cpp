// perspective_contraction_search.cpp -- finds the contraction-sensitive vector of tests/golden/perspective_rule.json
// (tools/make_perspective_golden.py builds and runs it):  g++ -O1 -std=c++17 -ffp-contract=off -o search perspective_contraction_search.cpp
//
// A NEAREST perspective view whose source column at one output pixel is k when every operation of the rule is rounded by itself, and
// k - 1 when the numerator's sum a0 xs + a1 ys, or the denominator's a6 xs + a7 ys, is contracted into one fused multiply-add
// (std::fma) -- alone or both.  Random a0, a1, a6, a7 and a pixel; a2 is then placed next to k den - (a0 xs + a1 ys), where the
// quotient sits on the integer k, and its neighbours are tried.  Prints the eight coefficients as hex floats, the pixel, and the two
// columns.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>

static double xin_of(const double* a, double xs, double ys, bool fuse_num, bool fuse_den) {
    const double q = a[1] * ys, k = a[7] * ys;
    const double pq = fuse_num ? std::fma(a[0], xs, q) : a[0] * xs + q;
    const double gk = fuse_den ? std::fma(a[6], xs, k) : a[6] * xs + k;
    return (pq + a[2]) / (gk + 1.0);
}

int main() {
    std::mt19937_64 rng(20261020);
    std::uniform_real_distribution<double> lin(0.6, 1.4), cross(-0.3, 0.3), proj(-0.02, 0.02);
    const int ow = 8, oh = 8, w = 12;
    for (long it = 0; it < 100000000L; ++it) {
        double a[8] = {lin(rng), cross(rng), 0.0, 0.0, 1.0, 0.0, proj(rng), proj(rng)};
        const int x = int(rng() % ow), y = int(rng() % oh);
        const double xs = x + 0.5, ys = y + 0.5;
        const double den = (a[6] * xs + a[7] * ys) + 1.0, pq = a[0] * xs + a[1] * ys;
        for (int k = 2; k < w - 1; ++k) {
            const double mid = double(k) * den - pq;
            for (double a2 : {std::nextafter(mid, -1e9), mid, std::nextafter(mid, 1e9)}) {
                a[2] = a2;
                const double u = xin_of(a, xs, ys, false, false);
                const double fn = xin_of(a, xs, ys, true, false), fd = xin_of(a, xs, ys, false, true), fb = xin_of(a, xs, ys, true, true);
                if (!(u >= 0 && fn >= 0 && fd >= 0 && fb >= 0)) continue;
                const int cu = int(u), cn = int(fn), cd = int(fd), cb = int(fb);
                if (cu == k && cn != cu && cd != cu && cb != cu && cn == cb && cd == cb) {
                    for (int i = 0; i < 8; ++i) std::printf("%a ", a[i]);
                    std::printf("%d %d %d %d\n", x, y, cu, cb);
                    return 0;
                }
            }
        }
    }
    return 1;
}
