// A stand-alone run of the calibration's host functions (csrc/calib_host.cpp, no device) for the host sanitizers:
//
//   g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude tools/calib_host_check.cpp lidar-slam-detection_amd/csrc/calib_host.cpp -o /tmp/calib_host_check && /tmp/calib_host_check
//
// Subsampling into heap arrays of exactly n bytes at n = 0 / 1 / 6001, the interpolation at both ends of a track held in exact-size heap
// arrays (with a start index at the last entry), and both optimisers on a quadratic with every evaluation checked against the box and the
// budget.  Exit status 0 and "ok" when all holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "lio_hip.h"

namespace {

struct Quad {
    const double *lb, *ub;
    int budget, calls, bad;
};

double quad(const double* x, int n, void* user) {
    Quad* q = static_cast<Quad*>(user);
    q->calls++;
    if (q->calls > q->budget) q->bad++;
    double s = 0.0;
    for (int i = 0; i < n; i++) {
        if (!(x[i] >= q->lb[i] && x[i] <= q->ub[i])) q->bad++;
        const double d = x[i] - (0.3 + 0.1 * i);
        s += (1.0 + 3.0 * i) * d * d;
    }
    return s;
}

}  // namespace

int main() {
    int bad = 0;
    for (uint64_t n : {0ull, 1ull, 6001ull}) {
        uint8_t* keep = n ? (uint8_t*)std::malloc(n) : nullptr;
        const int kept = lio_calib_subsample(n, 1700000000123456ll, keep);
        int count = 0;
        for (uint64_t i = 0; i < n; i++) count += keep[i];
        if (kept != count || (n == 1 && kept != 1) || (n == 6001 && !(kept > 5800 && kept <= 6001))) { std::printf("subsample n=%llu: %d kept\n", (unsigned long long)n, kept); bad++; }
        std::free(keep);
    }
    if (lio_calib_subsample(5, 0, nullptr) != LIO_E_INVALID) bad++;
    {
        const uint32_t m = 5;
        int64_t* stamps = (int64_t*)std::malloc(sizeof(int64_t) * m);
        float* T = (float*)std::malloc(sizeof(float) * 7 * m);
        for (uint32_t i = 0; i < m; i++) {
            stamps[i] = 1000000ll * i;
            const float v[6] = {1.0f * i, 0.5f * i, 0.f, 0.f, 0.f, 0.1f * i};
            lio_se3f_exp(v, T + 7 * i);
        }
        float out[7], v[6];
        uint32_t idx = 99;
        if (lio_calib_interpolate(stamps, T, m, -500000, 0, out, &idx) != LIO_OK || idx != 0) bad++;
        lio_se3f_log(out, v);
        if (!(std::fabs(v[0] + 0.5f) < 1e-5f && std::fabs(v[5] + 0.05f) < 1e-5f)) { std::printf("before the track: x %g yaw %g\n", v[0], v[5]); bad++; }
        if (lio_calib_interpolate(stamps, T, m, 4500000, 0, out, &idx) != LIO_OK || idx != m - 2) bad++;
        lio_se3f_log(out, v);
        if (!(std::fabs(v[0] - 4.5f) < 1e-4f && std::fabs(v[5] - 0.45f) < 1e-5f)) { std::printf("after the track: x %g yaw %g\n", v[0], v[5]); bad++; }
        if (lio_calib_interpolate(stamps, T, m, 500000, m - 1, out, &idx) != LIO_OK || idx != m - 2) bad++;  // the search cannot go back
        if (lio_calib_interpolate(stamps, T, 1, 0, 0, out, &idx) != LIO_E_STATE) bad++;
        std::free(stamps);
        std::free(T);
    }
    {
        const int n = 7;
        double* lb = (double*)std::malloc(sizeof(double) * n);
        double* ub = (double*)std::malloc(sizeof(double) * n);
        double* x0 = (double*)std::malloc(sizeof(double) * n);
        double* xb = (double*)std::malloc(sizeof(double) * n);
        for (int i = 0; i < n; i++) { lb[i] = -1.0 - i; ub[i] = 2.0 + i; x0[i] = 0.5 * (lb[i] + ub[i]); }
        lio_dfo_params p;
        lio_dfo_default_params(&p);
        lio_dfo_report rep;
        for (int budget : {1, 2, 17, 500}) {
            p.max_evals = budget;
            Quad q{lb, ub, budget, 0, 0};
            if (lio_dfo_direct_l(quad, &q, n, lb, ub, &p, nullptr, nullptr, xb, &rep) != LIO_OK || q.bad || rep.evals != q.calls) { std::printf("direct_l budget %d\n", budget); bad++; }
            Quad r{lb, ub, budget, 0, 0};
            if (lio_dfo_nelder_mead(quad, &r, n, x0, lb, ub, &p, nullptr, nullptr, xb, &rep) != LIO_OK || r.bad || rep.evals != r.calls) { std::printf("nelder_mead budget %d\n", budget); bad++; }
            if (budget == 500 && !(rep.f_best < 1e-6)) { std::printf("nelder_mead reached %g\n", rep.f_best); bad++; }
        }
        std::free(lb);
        std::free(ub);
        std::free(x0);
        std::free(xb);
    }
    std::printf(bad ? "FAILED (%d)\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
