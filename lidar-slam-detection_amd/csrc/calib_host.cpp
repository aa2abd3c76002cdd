// calib_host.cpp -- the host half of the lidar-INS calibration: plain C++, no device.
//
//   subsample    Scan::Scan (sensor_driver/calibration/lidar_ins/src/sensor.cpp:48-65): std::default_random_engine seeded with the stamp and
//                std::uniform_real_distribution<float>(0, 1) themselves, one draw per input point, kept iff draw < min(1, 6000 / (n + 1)).
//   se3f         Transform (lidar_ins/include/transform.h:23-65) in f32 with a quaternion and a translation, Eigen 3.3's statements written
//                out: Quaternionf(AngleAxisf), AngleAxisf(Quaternionf) (angle = 2 atan2(|v|, |w|), the axis' sign from w, (1, 0, 0) at zero),
//                toRotationMatrix, Quaternionf(Matrix3f), q * v as v + w (2 q x v) + q x (2 q x v), the scalar quaternion product.
//   interpolate  Odom::getOdomTransform (sensor.cpp:14-44): the forward-only search from start_idx, the step back, the ratio in f64 that is
//                not clamped (a stamp outside the track extrapolates) and is cast to f32 for the product with the f32 log vector.
//   dfo          DIRECT-L and Nelder-Mead over a box, restated from their published algorithms (the reference calls nlopt's GN_DIRECT_L and
//                LN_BOBYQA, which this project cannot build or pin): Jones, Perttunen & Stuckman (1993) with Gablonsky & Kelley's (2001)
//                locally biased selection -- the measure of a rectangle is its longest side, and among the rectangles of one measure only the
//                one with the smallest f is a candidate; Nelder & Mead (1965) with coefficients 1, 2, 1/2, 1/2 and every point projected onto
//                the box.
#include "calib_host.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <random>
#include <vector>

namespace lio {
namespace calib {

namespace {

inline void cross(const float a[3], const float b[3], float o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// Eigen's QuaternionBase::_transformVector
inline void rotate(const float q[4], const float v[3], float o[3]) {
    float uv[3], c[3];
    cross(q + 1, v, uv);
    for (int i = 0; i < 3; i++) uv[i] += uv[i];
    cross(q + 1, uv, c);
    for (int i = 0; i < 3; i++) o[i] = v[i] + q[0] * uv[i] + c[i];
}

inline void qmul(const float a[4], const float b[4], float o[4]) {
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
    o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}

inline float norm3(const float v[3]) { return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

}  // namespace

Se3f se3_identity() { return Se3f{{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f, 0.f}}; }

Se3f se3_exp(const float v[6]) {
    constexpr float kEpsilon = 1e-8f;
    Se3f o = se3_identity();
    for (int i = 0; i < 3; i++) o.t[i] = v[i];
    const float norm = norm3(v + 3);
    if (norm < kEpsilon) return o;
    const float ha = 0.5f * norm, s = std::sin(ha);
    o.q[0] = std::cos(ha);
    for (int i = 0; i < 3; i++) o.q[1 + i] = s * (v[3 + i] / norm);
    return o;
}

void se3_log(const Se3f& a, float v[6]) {
    for (int i = 0; i < 3; i++) v[i] = a.t[i];
    float n = norm3(a.q + 1);
    if (n < std::numeric_limits<float>::epsilon()) {  // Eigen falls back to stableNorm: the same value without the underflow of the squares
        const float m = std::max(std::fabs(a.q[1]), std::max(std::fabs(a.q[2]), std::fabs(a.q[3])));
        if (m > 0.f) {
            const float s[3] = {a.q[1] / m, a.q[2] / m, a.q[3] / m};
            n = m * norm3(s);
        } else {
            n = 0.f;
        }
    }
    if (n != 0.f) {
        const float angle = 2.f * std::atan2(n, std::fabs(a.q[0]));
        if (a.q[0] < 0.f) n = -n;
        for (int i = 0; i < 3; i++) v[3 + i] = angle * (a.q[1 + i] / n);
    } else {
        v[3] = v[4] = v[5] = 0.f;  // angle 0 times the axis (1, 0, 0)
    }
}

Se3f se3_mul(const Se3f& a, const Se3f& b) {
    Se3f o;
    float r[3];
    rotate(a.q, b.t, r);
    for (int i = 0; i < 3; i++) o.t[i] = a.t[i] + r[i];
    qmul(a.q, b.q, o.q);
    return o;
}

Se3f se3_inverse(const Se3f& a) {
    Se3f o;
    o.q[0] = a.q[0];
    for (int i = 1; i < 4; i++) o.q[i] = -a.q[i];
    float r[3];
    rotate(o.q, a.t, r);
    for (int i = 0; i < 3; i++) o.t[i] = -r[i];
    return o;
}

void se3_matrix(const Se3f& a, float M[16]) {
    const float w = a.q[0], x = a.q[1], y = a.q[2], z = a.q[3];
    const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w;
    const float txx = tx * x, txy = ty * x, txz = tz * x;
    const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
    M[0] = 1.f - (tyy + tzz); M[1] = txy - twz;         M[2] = txz + twy;          M[3] = a.t[0];
    M[4] = txy + twz;         M[5] = 1.f - (txx + tzz); M[6] = tyz - twx;          M[7] = a.t[1];
    M[8] = txz - twy;         M[9] = tyz + twx;         M[10] = 1.f - (txx + tyy); M[11] = a.t[2];
    M[12] = M[13] = M[14] = 0.f;
    M[15] = 1.f;
}

Se3f se3_from_matrix(const float M[16]) {
    Se3f o;
    o.t[0] = M[3]; o.t[1] = M[7]; o.t[2] = M[11];
    auto m = [&](int r, int c) { return M[4 * r + c]; };
    float t = m(0, 0) + m(1, 1) + m(2, 2);
    if (t > 0.f) {
        t = std::sqrt(t + 1.f);
        o.q[0] = 0.5f * t;
        t = 0.5f / t;
        o.q[1] = (m(2, 1) - m(1, 2)) * t;
        o.q[2] = (m(0, 2) - m(2, 0)) * t;
        o.q[3] = (m(1, 0) - m(0, 1)) * t;
    } else {
        int i = 0;
        if (m(1, 1) > m(0, 0)) i = 1;
        if (m(2, 2) > m(i, i)) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m(i, i) - m(j, j) - m(k, k) + 1.f);
        o.q[1 + i] = 0.5f * t;
        t = 0.5f / t;
        o.q[0] = (m(k, j) - m(j, k)) * t;
        o.q[1 + j] = (m(j, i) + m(i, j)) * t;
        o.q[1 + k] = (m(k, i) + m(i, k)) * t;
    }
    return o;
}

Se3f interpolate(const int64_t* stamps, const Se3f* T, uint32_t m, int64_t stamp, uint32_t start_idx, uint32_t* match_idx) {
    uint64_t idx = start_idx;
    while (idx < (uint64_t)m - 1 && stamp > stamps[idx]) ++idx;
    if (idx > 0) --idx;
    if (idx > (uint64_t)m - 2) idx = m - 2;  // a start_idx past the track: the reference would read past its vector
    if (match_idx) *match_idx = (uint32_t)idx;
    const double ratio = static_cast<double>(stamp - stamps[idx]) / static_cast<double>(stamps[idx + 1] - stamps[idx]);
    float d[6];
    se3_log(se3_mul(se3_inverse(T[idx]), T[idx + 1]), d);
    const float r = (float)ratio;
    for (int i = 0; i < 6; i++) d[i] = r * d[i];
    return se3_mul(T[idx], se3_exp(d));
}

}  // namespace calib
}  // namespace lio

using namespace lio::calib;

namespace {

inline Se3f load7(const float* p) { return Se3f{{p[0], p[1], p[2]}, {p[3], p[4], p[5], p[6]}}; }
inline void store7(const Se3f& a, float* p) {
    for (int i = 0; i < 3; i++) p[i] = a.t[i];
    for (int i = 0; i < 4; i++) p[3 + i] = a.q[i];
}

struct Evaluator {
    lio_dfo_fn f;
    void* user;
    int n;
    const double *lb, *ub;
    int budget;
    lio_dfo_hook hook;
    void* hook_user;
    int evals = 0;
    bool stopped = false;
    double f_best = std::numeric_limits<double>::infinity();
    std::vector<double> x_best;

    bool spent() const { return stopped || evals >= budget; }
    // x is clamped onto the box in place; false: not evaluated (budget spent or the hook asked to stop)
    bool eval(double* x, double* out) {
        if (spent()) return false;
        for (int i = 0; i < n; i++) x[i] = std::min(std::max(x[i], lb[i]), ub[i]);
        const double v = f(x, n, user);
        evals++;
        if (x_best.empty() || v < f_best) {
            f_best = v;
            x_best.assign(x, x + n);
        }
        if (hook && hook(evals, x, n, v, hook_user)) stopped = true;
        *out = v;
        return true;
    }
};

bool box_ok(int n, const double* lb, const double* ub) {
    if (n < 1 || n > LIO_DFO_MAX_DIM || !lb || !ub) return false;
    for (int i = 0; i < n; i++)
        if (!(std::isfinite(lb[i]) && std::isfinite(ub[i]) && lb[i] <= ub[i])) return false;
    return true;
}

void finish(const Evaluator& E, int stop, double* x_best, lio_dfo_report* rep) {
    if (x_best && !E.x_best.empty()) std::copy(E.x_best.begin(), E.x_best.end(), x_best);
    if (rep) {
        rep->evals = E.evals;
        rep->stop = E.stopped ? LIO_DFO_STOP_HOOK : stop;
        rep->f_best = E.f_best;
    }
}

struct Rect {
    double c[LIO_DFO_MAX_DIM];       // centre in the unit cube
    uint8_t level[LIO_DFO_MAX_DIM];  // trisections per coordinate: the side is 3^-level
    double f;
};

}  // namespace

extern "C" {

int lio_calib_subsample(uint64_t n, int64_t stamp_us, uint8_t* keep) {
    if (n && !keep) return LIO_E_INVALID;
    if (n > 0x7FFFFFFFull) return LIO_E_CAPACITY;
    std::default_random_engine generator(stamp_us);
    std::uniform_real_distribution<float> distribution(0, 1);
    const float keep_points_ratio = std::min(1.0f, (float(6000) / (n + 1)));
    int kept = 0;
    for (uint64_t i = 0; i < n; i++) {
        keep[i] = distribution(generator) < keep_points_ratio ? 1 : 0;
        kept += keep[i];
    }
    return kept;
}

void lio_se3f_exp(const float v[6], float T[7]) { store7(se3_exp(v), T); }
void lio_se3f_log(const float T[7], float v[6]) { se3_log(load7(T), v); }
void lio_se3f_mul(const float a[7], const float b[7], float o[7]) { store7(se3_mul(load7(a), load7(b)), o); }
void lio_se3f_inverse(const float a[7], float o[7]) { store7(se3_inverse(load7(a)), o); }
void lio_se3f_matrix(const float a[7], float M[16]) { se3_matrix(load7(a), M); }
void lio_se3f_from_matrix(const float M[16], float T[7]) { store7(se3_from_matrix(M), T); }

int lio_calib_interpolate(const int64_t* stamps, const float* T, uint32_t m, int64_t stamp, uint32_t start_idx, float T_out[7], uint32_t* match_idx) {
    if (!stamps || !T || !T_out) return LIO_E_INVALID;
    if (m < 2) return LIO_E_STATE;
    std::vector<Se3f> tr(m);
    for (uint32_t i = 0; i < m; i++) tr[i] = load7(T + 7ull * i);
    store7(interpolate(stamps, tr.data(), m, stamp, start_idx, match_idx), T_out);
    return LIO_OK;
}

void lio_dfo_default_params(lio_dfo_params* p) {
    if (!p) return;
    p->max_evals = 500;
    p->reserved = 0;
    p->xtol_abs = 1e-4;
    p->epsilon = 1e-4;
    for (int i = 0; i < LIO_DFO_MAX_DIM; i++) p->step[i] = 0.0;  // 0: a twentieth of the box's side
}

int lio_dfo_direct_l(lio_dfo_fn f, void* user, int n, const double* lb, const double* ub, const lio_dfo_params* p, lio_dfo_hook hook, void* hook_user,
                     double* x_best, lio_dfo_report* rep) {
    if (!f || !p || !box_ok(n, lb, ub) || p->max_evals < 1 || !(p->epsilon >= 0.0) || !(p->xtol_abs >= 0.0)) return LIO_E_INVALID;
    Evaluator E{f, user, n, lb, ub, p->max_evals, hook, hook_user};
    auto real = [&](const double* c, double* x) {
        for (int i = 0; i < n; i++) x[i] = lb[i] + c[i] * (ub[i] - lb[i]);
    };
    std::vector<Rect> rects;
    rects.reserve((size_t)p->max_evals + 1);
    double x[LIO_DFO_MAX_DIM];
    {
        Rect r{};
        for (int i = 0; i < n; i++) r.c[i] = 0.5;
        real(r.c, x);
        if (!E.eval(x, &r.f)) { finish(E, LIO_DFO_STOP_EVALS, x_best, rep); return LIO_OK; }
        rects.push_back(r);
    }
    int stop = LIO_DFO_STOP_EVALS;
    std::vector<int> best_of;  // by measure (the smallest level of a rectangle): the index of its smallest f, -1 none
    std::vector<int> chosen;
    while (!E.spent()) {
        // one candidate per measure
        best_of.assign(256, -1);
        int lmax = 0;
        for (size_t j = 0; j < rects.size(); j++) {
            int lv = 255;
            for (int i = 0; i < n; i++) lv = std::min<int>(lv, rects[j].level[i]);
            lmax = std::max(lmax, lv);
            if (best_of[lv] < 0 || rects[j].f < rects[best_of[lv]].f) best_of[lv] = (int)j;
        }
        // the potentially optimal ones: on the lower right hull of (side, f), and better than fmin - eps |fmin| for the largest rate K allowed
        const double fmin = E.f_best;
        chosen.clear();
        for (int lv = 0; lv <= lmax; lv++) {
            const int j = best_of[lv];
            if (j < 0) continue;
            const double dj = std::pow(3.0, -lv), fj = rects[j].f;
            double klo = 0.0, khi = std::numeric_limits<double>::infinity();
            bool ok = true;
            for (int lo = 0; lo <= lmax && ok; lo++) {
                const int i = best_of[lo];
                if (i < 0 || lo == lv) continue;
                const double di = std::pow(3.0, -lo), fi = rects[i].f;
                if (di > dj) khi = std::min(khi, (fi - fj) / (di - dj));
                else klo = std::max(klo, (fj - fi) / (dj - di));
            }
            if (!(klo <= khi) || !(khi > 0.0)) ok = false;
            if (ok && std::isfinite(khi) && !(fj - khi * dj <= fmin - p->epsilon * std::fabs(fmin))) ok = false;
            if (ok) chosen.push_back(j);
        }
        if (chosen.empty()) chosen.push_back(best_of[0] >= 0 ? best_of[0] : 0);  // cannot happen: the largest measure always qualifies
        bool divided = false;
        for (size_t cj = 0; cj < chosen.size() && !E.spent(); cj++) {
            const int j = chosen[cj];
            int lv = 255;
            for (int i = 0; i < n; i++) lv = std::min<int>(lv, rects[j].level[i]);
            const double side = std::pow(3.0, -lv);
            bool small = true;
            for (int i = 0; i < n; i++) small = small && side * (ub[i] - lb[i]) <= p->xtol_abs;
            if (small) continue;
            if (lv >= 200) continue;
            // sample c +- side / 3 along every longest side
            const double delta = side / 3.0;
            int dims[LIO_DFO_MAX_DIM], nd = 0;
            double fp[LIO_DFO_MAX_DIM], fm[LIO_DFO_MAX_DIM];
            Rect rp[LIO_DFO_MAX_DIM], rm[LIO_DFO_MAX_DIM];
            bool complete = true;
            for (int i = 0; i < n && complete; i++) {
                if (rects[j].level[i] != lv) continue;
                Rect a = rects[j], b = rects[j];
                a.c[i] += delta;
                b.c[i] -= delta;
                real(a.c, x);
                if (!E.eval(x, &a.f)) { complete = false; break; }
                real(b.c, x);
                if (!E.eval(x, &b.f)) { complete = false; break; }
                dims[nd] = i;
                fp[nd] = a.f;
                fm[nd] = b.f;
                rp[nd] = a;
                rm[nd] = b;
                nd++;
            }
            if (!complete) break;  // the budget ran out in the middle of a rectangle: its samples count for the best point only
            // trisect in ascending order of w_i = min(f+, f-): the best samples keep the largest rectangles
            int order[LIO_DFO_MAX_DIM];
            for (int i = 0; i < nd; i++) order[i] = i;
            std::stable_sort(order, order + nd, [&](int a, int b) { return std::min(fp[a], fm[a]) < std::min(fp[b], fm[b]); });
            for (int s = 0; s < nd; s++) {
                const int d = dims[order[s]];
                rects[j].level[d]++;
                for (int t = s; t < nd; t++) {  // the children of the later cuts inherit this cut
                    rp[order[t]].level[d]++;
                    rm[order[t]].level[d]++;
                }
            }
            for (int s = 0; s < nd; s++) {
                rects.push_back(rp[s]);
                rects.push_back(rm[s]);
            }
            divided = true;
        }
        if (!divided && !E.spent()) { stop = LIO_DFO_STOP_XTOL; break; }
    }
    finish(E, stop, x_best, rep);
    return LIO_OK;
}

int lio_dfo_nelder_mead(lio_dfo_fn f, void* user, int n, const double* x0, const double* lb, const double* ub, const lio_dfo_params* p, lio_dfo_hook hook,
                        void* hook_user, double* x_best, lio_dfo_report* rep) {
    if (!f || !p || !x0 || !box_ok(n, lb, ub) || p->max_evals < 1 || !(p->xtol_abs >= 0.0)) return LIO_E_INVALID;
    for (int i = 0; i < n; i++)
        if (!std::isfinite(x0[i])) return LIO_E_INVALID;
    Evaluator E{f, user, n, lb, ub, p->max_evals, hook, hook_user};
    const int m = n + 1;
    std::vector<double> X((size_t)m * n), F(m);
    int stop = LIO_DFO_STOP_EVALS;
    bool ok = true;
    for (int v = 0; v < m && ok; v++) {
        double* xv = &X[(size_t)v * n];
        for (int i = 0; i < n; i++) xv[i] = std::min(std::max(x0[i], lb[i]), ub[i]);
        if (v > 0) {
            const int i = v - 1;
            double h = p->step[i] != 0.0 ? p->step[i] : 0.05 * (ub[i] - lb[i]);
            if (xv[i] + h > ub[i]) h = -h;  // the step that stays inside
            xv[i] += h;
        }
        ok = E.eval(xv, &F[v]);
    }
    std::vector<int> idx(m);
    std::vector<double> cen(n), xr(n), xe(n), xc(n);
    while (ok && !E.spent()) {
        for (int v = 0; v < m; v++) idx[v] = v;
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return F[a] < F[b]; });
        const int lo = idx[0], hi = idx[m - 1], nhi = idx[m - 2];
        bool small = true;
        for (int v = 1; v < m && small; v++)
            for (int i = 0; i < n; i++) small = small && std::fabs(X[(size_t)idx[v] * n + i] - X[(size_t)lo * n + i]) <= p->xtol_abs;
        if (small) { stop = LIO_DFO_STOP_XTOL; break; }
        for (int i = 0; i < n; i++) {
            double s = 0.0;
            for (int v = 0; v < m - 1; v++) s += X[(size_t)idx[v] * n + i];
            cen[i] = s / n;
        }
        double* xh = &X[(size_t)hi * n];
        double fr, fe, fc;
        for (int i = 0; i < n; i++) xr[i] = cen[i] + (cen[i] - xh[i]);
        if (!E.eval(xr.data(), &fr)) break;
        if (fr < F[lo]) {
            for (int i = 0; i < n; i++) xe[i] = cen[i] + 2.0 * (cen[i] - xh[i]);
            if (!E.eval(xe.data(), &fe)) { std::copy(xr.begin(), xr.end(), xh); F[hi] = fr; break; }
            if (fe < fr) { std::copy(xe.begin(), xe.end(), xh); F[hi] = fe; }
            else { std::copy(xr.begin(), xr.end(), xh); F[hi] = fr; }
            continue;
        }
        if (fr < F[nhi]) { std::copy(xr.begin(), xr.end(), xh); F[hi] = fr; continue; }
        bool shrink;
        if (fr < F[hi]) {  // outside contraction
            for (int i = 0; i < n; i++) xc[i] = cen[i] + 0.5 * (xr[i] - cen[i]);
            if (!E.eval(xc.data(), &fc)) break;
            shrink = !(fc <= fr);
        } else {  // inside contraction
            for (int i = 0; i < n; i++) xc[i] = cen[i] - 0.5 * (cen[i] - xh[i]);
            if (!E.eval(xc.data(), &fc)) break;
            shrink = !(fc < F[hi]);
        }
        if (!shrink) { std::copy(xc.begin(), xc.end(), xh); F[hi] = fc; continue; }
        for (int v = 1; v < m; v++) {
            double* xv = &X[(size_t)idx[v] * n];
            for (int i = 0; i < n; i++) xv[i] = X[(size_t)lo * n + i] + 0.5 * (xv[i] - X[(size_t)lo * n + i]);
            if (!E.eval(xv, &F[idx[v]])) { ok = false; break; }
        }
    }
    finish(E, stop, x_best, rep);
    return LIO_OK;
}

}  // extern "C"
