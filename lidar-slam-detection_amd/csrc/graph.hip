// graph.hip -- the pose graph on gfx950 (wave64): SE3 nodes, EdgeSE3 edges, Huber, Levenberg-Marquardt with a block-Jacobi conjugate-gradient
// solve; include/lio_hip.h states the rules (restated from g2o's published source: g2o is not in the tree).
//
//   state      nodes {t, unit q} and edges {from, to, M as t + q, information, kernel, delta, live} resident in HBM; the host keeps the topology
//              (ends, live, fixed) and rebuilds three CSRs when it changes: node -> incident edges (diagonal blocks and b), node pair -> edges
//              (off-diagonal blocks), block row -> (column, block, transposed) for the matrix-vector product
//   linearise  graph_linearize: one lane per edge (grid-stride): e, chi2, rho', the two Jacobians, J^T W J for (i,i), (i,j), (j,j), -J^T W e
//   assemble   graph_assemble: one lane per entry of a block; a block is the sum of its edges' entries in rising edge id: no atomics
//   solve      graph_solve: ONE workgroup runs the whole preconditioned CG of a trial: vectors in global memory, scalar rows strided over the
//              lanes, dot products folded in a fixed order, __syncthreads between the phases; no grid-wide barrier
//   update     graph_update (backup + X <- X fromVectorMQT(d), q renormalised), graph_chi2 (rho per edge, one partial per 256 edges),
//              graph_decide (one workgroup: folds the partials in order, the LM bookkeeping, restores a rejected trial)
//   priors     unary 3-row edges (GNSS position, orientation, floor plane) live in a compact array of their own (PriorDev); a prior takes
//              the next id of the one edge counter, and the edge array keeps a placeholder (live = kPriorSlot, from = the prior's index) at
//              that id.  graph_linearize_prior (one lane per prior) writes e, chi2, rho', J^T W J and -J^T W e into the id's Hii / bi slots, so
//              graph_assemble and the node -> edges lists take both kinds in rising id as they are; graph_chi2<true> follows the placeholder,
//              so a prior's rho joins the partial of its 256 ids.  Without priors neither the extra launch nor graph_chi2<true> is used.
//   moment     between lio_graph_moment_begin and _end every live XYZ prior is an EdgeSE3GNSS to one shared 3-DoF vertex m, a dense border of three
//              unknowns on the system.  graph_linearize_moment (after graph_linearize_prior) takes those priors' slots again and leaves the 6 x 3
//              coupling block, the 3 x 3 and the 3 of b per prior; graph_assemble_border sums them per active node and over all, in rising id,
//              and adds the moment's own prior; graph_solve_border is graph_solve's text with the border compiled in (three more rows, the
//              damped 3 x 3's inverse in the preconditioner, three more block sums per product); graph_update_moment, graph_chi2_moment and
//              graph_decide_moment carry m through the trial.  With no stage open none of these is launched and the kernels above take the
//              arguments they always took.
// The host enqueues, per LM iteration, linearise + assemble + kMaxTrials trials; a kernel whose trial is not wanted (the iteration was decided, or
// the optimisation stopped) leaves at once.  The host reads one LmState per iteration.
#include <cfloat>
#include <cmath>
#include <map>
#include <utility>
#include <vector>

#include "lio_common.h"

namespace lio {
namespace graph {

constexpr int kSolveThreads = 1024;
constexpr int kEdgeThreads = 256;
constexpr int kMaxTrials = 10;   // _maxTrialsAfterFailure
constexpr int kEvents = 2 * kMaxTrials + 3;

struct EdgeDev {
    int32_t from, to, kernel, live;
    double delta;
    double mt[3], mq[4];  // the measurement: translation, unit quaternion (x, y, z, w)
    double info[36];
};

// a unary edge on one node: LIO_GRAPH_PRIOR_*; m = xyz / unit quaternion (x, y, z, w >= 0) / unit plane (n, d); plane = the world plane of PLANE
struct PriorDev {
    int32_t node, type, kernel, live;
    int32_t id, pad;  // its edge id
    double delta;
    double m[4], plane[4];
    double info[9];
};
constexpr int32_t kPriorSlot = 2;  // EdgeDev::live of the placeholder a prior leaves in the edge array; EdgeDev::from is then the prior's index

struct LmState {
    double lambda, nu, chi2, chi2_new, rho, scale, cg_relres;
    int32_t batch;             // the LM iteration whose trials are wanted (the host's launch tag)
    int32_t iteration;         // iterations done
    int32_t trials;            // qmax of the current iteration
    int32_t stop;              // LIO_GRAPH_STOP_*
    int32_t need_lambda_init;
    int32_t solve_ok;
    int32_t cg_iterations, cg_total, total_trials, accepted;
};

// what a per-edge linearisation leaves: offsets into one allocation of cap edges
struct LinBuf {
    double *err, *chi2, *rho1, *Ji, *Jj, *Hii, *Hij, *Hjj, *bi, *bj;
};

#define HD __host__ __device__ inline

HD void q_mul(const double a[4], const double b[4], double o[4]) {
    o[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    o[1] = ((a[3] * b[1] - a[0] * b[2]) + a[1] * b[3]) + a[2] * b[0];
    o[2] = ((a[3] * b[2] + a[0] * b[1]) - a[1] * b[0]) + a[2] * b[3];
    o[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
}
HD void q_normalise(double q[4]) {
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}
// Eigen's Quaternion::toRotationMatrix, row-major
HD void q_to_R(const double q[4], double R[9]) {
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
// Eigen's Quaternion(Matrix3) of the rotation of a row-major 4 x 4, then normalised
inline void T_to_tq(const double T[16], double t[3], double q[4]) {
    t[0] = T[3]; t[1] = T[7]; t[2] = T[11];
    const double tr = T[0] + T[5] + T[10];
    if (tr > 0) {
        double s = sqrt(tr + 1.0);
        q[3] = 0.5 * s; s = 0.5 / s;
        q[0] = (T[9] - T[6]) * s; q[1] = (T[2] - T[8]) * s; q[2] = (T[4] - T[1]) * s;
    } else {
        int i = 0;
        if (T[5] > T[0]) i = 1;
        if (T[10] > T[i * 5]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double s = sqrt(T[i * 5] - T[j * 5] - T[k * 5] + 1.0);
        q[i] = 0.5 * s; s = 0.5 / s;
        q[3] = (T[k * 4 + j] - T[j * 4 + k]) * s;
        q[j] = (T[j * 4 + i] + T[i * 4 + j]) * s;
        q[k] = (T[k * 4 + i] + T[i * 4 + k]) * s;
    }
    q_normalise(q);
}
inline void tq_to_T(const double t[3], const double q[4], double T[16]) {
    double R[9];
    q_to_R(q, R);
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T[r * 4 + c] = R[r * 3 + c]; T[r * 4 + 3] = t[r]; }
    T[12] = T[13] = T[14] = 0.0; T[15] = 1.0;
}

// e = toVectorMQT(M^-1 Xi^-1 Xj); also what the Jacobians need: tb, qb of Xi^-1 Xj, the error quaternion (normalised, w >= 0)
HD void edge_eval(const double ti[3], const double qi[4], const double tj[3], const double qj[4], const double mt[3], const double mq[4], double e[6],
                  double tb[3], double qb[4], double qe[4]) {
    double R[9];
    q_to_R(qi, R);
    const double d[3] = {tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]};
#pragma unroll
    for (int c = 0; c < 3; c++) tb[c] = (R[c] * d[0] + R[3 + c] * d[1]) + R[6 + c] * d[2];
    const double qic[4] = {-qi[0], -qi[1], -qi[2], qi[3]};
    q_mul(qic, qj, qb);
    q_to_R(mq, R);
    const double u[3] = {tb[0] - mt[0], tb[1] - mt[1], tb[2] - mt[2]};
#pragma unroll
    for (int c = 0; c < 3; c++) e[c] = (R[c] * u[0] + R[3 + c] * u[1]) + R[6 + c] * u[2];
    const double qmc[4] = {-mq[0], -mq[1], -mq[2], mq[3]};
    q_mul(qmc, qb, qe);
    q_normalise(qe);
    if (qe[3] < 0) { qe[0] = -qe[0]; qe[1] = -qe[1]; qe[2] = -qe[2]; qe[3] = -qe[3]; }
    e[3] = qe[0]; e[4] = qe[1]; e[5] = qe[2];
}

// chi2 = e^T Omega e and Huber: rho, rho'
HD double edge_chi2(const double e[6], const double* __restrict__ info, double We[6]) {
    double chi2 = 0.0;
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) s += info[r * 6 + c] * e[c];
        We[r] = s;
        chi2 += e[r] * s;
    }
    return chi2;
}
HD void robustify(double chi2, int kernel, double delta, double* rho, double* rho1) {
    *rho = chi2; *rho1 = 1.0;
    if (kernel == LIO_GRAPH_KERNEL_HUBER) {
        const double s = sqrt(chi2);
        if (!(s <= delta)) { *rho = 2.0 * delta * s - delta * delta; *rho1 = delta / s; }
    } else if (kernel == LIO_GRAPH_KERNEL_DCS2) {  // RobustKernelDCS2: phi = delta
        const double p = delta + chi2, s = (2.0 * delta) / p;
        if (!(s >= 1.0)) { *rho = s * chi2 * s; *rho1 = (4.0 * delta * delta * (delta - chi2)) / (p * p * p); }
    }
}

HD double az_of(const double x[3]) { return atan2(x[1], x[0]); }
HD double el_of(const double x[3]) { return atan2(x[2], hypot(x[0], x[1])); }
// the error of a prior on the node (t, q); for PLANE also what its Jacobian needs: A = Rz(az(n_m)) Ry(-el(n_m)) row-major, n_l = R^T n, u = A^T n_l;
// for QUAT sgn = the sign that brought q to the measurement's side
HD void prior_eval(int type, const double t[3], const double q[4], const double m[4], const double plane[4], double e[3], double A[9], double nl[3], double u[3],
                   double* sgn) {
    if (type == LIO_GRAPH_PRIOR_XYZ) {
        e[0] = t[0] - m[0]; e[1] = t[1] - m[1]; e[2] = t[2] - m[2];
    } else if (type == LIO_GRAPH_PRIOR_QUAT) {
        const double s = (((m[0] * q[0] + m[1] * q[1]) + m[2] * q[2]) + m[3] * q[3]) < 0 ? -1.0 : 1.0;
        *sgn = s;
        e[0] = s * q[0] - m[0]; e[1] = s * q[1] - m[1]; e[2] = s * q[2] - m[2];
    } else {
        double R[9];
        q_to_R(q, R);
#pragma unroll
        for (int c = 0; c < 3; c++) nl[c] = (R[c] * plane[0] + R[3 + c] * plane[1]) + R[6 + c] * plane[2];
        const double dl = plane[3] + ((t[0] * plane[0] + t[1] * plane[1]) + t[2] * plane[2]);
        // cos and sin of az(n_m) and el(n_m) of the unit normal, without the angles: el's are (h, m_z), az's (m_x, m_y) / h, and (1, 0) when h = 0
        const double h = hypot(m[0], m[1]);
        const double cb = h, sb = m[2], ca = h > 0 ? m[0] / h : 1.0, sa = h > 0 ? m[1] / h : 0.0;
        A[0] = ca * cb; A[1] = -sa; A[2] = -ca * sb;
        A[3] = sa * cb; A[4] = ca;  A[5] = -sa * sb;
        A[6] = sb;      A[7] = 0.0; A[8] = cb;
#pragma unroll
        for (int c = 0; c < 3; c++) u[c] = (A[c] * nl[0] + A[3 + c] * nl[1]) + A[6 + c] * nl[2];
        e[0] = az_of(u); e[1] = el_of(u); e[2] = m[3] - dl;
    }
}
HD double prior_chi2(const double e[3], const double* __restrict__ info, double We[3]) {
    double chi2 = 0.0;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double s = (info[r * 3] * e[0] + info[r * 3 + 1] * e[1]) + info[r * 3 + 2] * e[2];
        We[r] = s;
        chi2 += e[r] * s;
    }
    return chi2;
}
// rho of a live prior at the current estimate
HD double prior_rho(const PriorDev& pr, const double* __restrict__ nt, const double* __restrict__ nq) {
    double t[3], q[4], m[4], pl[4], e[3], A[9], nl[3], u[3], We[3], sgn = 1.0, rho, rho1;
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = nt[pr.node * 3ull + k];
#pragma unroll
    for (int k = 0; k < 4; k++) { q[k] = nq[pr.node * 4ull + k]; m[k] = pr.m[k]; pl[k] = pr.plane[k]; }
    prior_eval(pr.type, t, q, m, pl, e, A, nl, u, &sgn);
    robustify(prior_chi2(e, pr.info, We), pr.kernel, pr.delta, &rho, &rho1);
    return rho;
}
// the moment stage's state on the device: the moment m, its backup, the information of its prior at 0
constexpr int kMomM = 0, kMomBak = 3, kMomInfo = 6, kMomDoubles = 15;
// what graph_linearize_moment leaves per prior (by its index, not its id): the 6 x 3 coupling block, the border's 3 x 3 and its 3 of b
constexpr int kMlinHpm = 0, kMlinHmm = 18, kMlinBm = 27, kMlinDoubles = 30;
// EdgeSE3GNSS: e = t - (z + R m) for the node (t, R), the measurement z and the moment m
HD void moment_eval(const double t[3], const double R[9], const double z[3], const double m[3], double e[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) e[r] = t[r] - (z[r] + ((R[r * 3] * m[0] + R[r * 3 + 1] * m[1]) + R[r * 3 + 2] * m[2]));
}
// rho of a live XYZ prior taken as a moment edge
HD double moment_rho(const PriorDev& pr, const double* __restrict__ nt, const double* __restrict__ nq, const double* __restrict__ mom) {
    double t[3], q[4], z[3], m[3], R[9], e[3], We[3], rho, rho1;
#pragma unroll
    for (int k = 0; k < 3; k++) { t[k] = nt[pr.node * 3ull + k]; z[k] = pr.m[k]; m[k] = mom[kMomM + k]; }
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = nq[pr.node * 4ull + k];
    q_to_R(q, R);
    moment_eval(t, R, z, m, e);
    robustify(prior_chi2(e, pr.info, We), pr.kernel, pr.delta, &rho, &rho1);
    return rho;
}
// m^T Omega m of the moment's own prior (EdgeXYZPrior at 0, no kernel)
HD double moment_prior_chi2(const double m[3], const double* __restrict__ info) {
    double We[3];
    return prior_chi2(m, info, We);
}
// X <- X fromVectorMQT(d), the quaternion renormalised
HD void apply_delta(double t[3], double q[4], const double d[6]) {
    double R[9];
    q_to_R(q, R);
#pragma unroll
    for (int r = 0; r < 3; r++) t[r] += (R[r * 3] * d[0] + R[r * 3 + 1] * d[1]) + R[r * 3 + 2] * d[2];
    const double w2 = 1.0 - ((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]);
    if (w2 < 0) return;  // the identity rotation
    const double dq[4] = {d[3], d[4], d[5], sqrt(w2)};
    double o[4];
    q_mul(q, dq, o);
    q_normalise(o);
    q[0] = o[0]; q[1] = o[1]; q[2] = o[2]; q[3] = o[3];
}

__device__ inline bool wanted(const LmState* st, int tag) { return tag < 0 || (st->stop == 0 && st->batch == tag); }

// O = A^T B for 6 x 6 row-major register arrays, written straight out
__device__ inline void atb_store(const double A[36], const double B[36], double* __restrict__ out) {
#pragma unroll
    for (int r = 0; r < 6; r++) {
#pragma unroll
        for (int c = 0; c < 6; c++) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) s += A[k * 6 + r] * B[k * 6 + c];
            out[r * 6 + c] = s;
        }
    }
}

__global__ void __launch_bounds__(kEdgeThreads) graph_linearize(const EdgeDev* __restrict__ edges, uint32_t E, const double* __restrict__ nt,
                                                                const double* __restrict__ nq, const LmState* __restrict__ st, int tag, LinBuf L) {
    if (!wanted(st, tag)) return;
    for (uint32_t id = blockIdx.x * kEdgeThreads + threadIdx.x; id < E; id += gridDim.x * kEdgeThreads) {
        const EdgeDev& ed = edges[id];
        if (ed.live != 1) {  // removed, or a prior's placeholder: graph_linearize_prior fills a live prior's slots after this kernel
#pragma unroll
            for (int k = 0; k < 6; k++) L.err[id * 6ull + k] = 0.0;
            L.chi2[id] = 0.0; L.rho1[id] = 0.0;
            continue;
        }
        double ti[3], qi[4], tj[3], qj[4], mt[3], mq[4];
#pragma unroll
        for (int k = 0; k < 3; k++) { ti[k] = nt[ed.from * 3ull + k]; tj[k] = nt[ed.to * 3ull + k]; mt[k] = ed.mt[k]; }
#pragma unroll
        for (int k = 0; k < 4; k++) { qi[k] = nq[ed.from * 4ull + k]; qj[k] = nq[ed.to * 4ull + k]; mq[k] = ed.mq[k]; }
        double e[6], tb[3], qb[4], qe[4], We[6];
        edge_eval(ti, qi, tj, qj, mt, mq, e, tb, qb, qe);
        const double chi2 = edge_chi2(e, ed.info, We);
        double rho, rho1;
        robustify(chi2, ed.kernel, ed.delta, &rho, &rho1);
#pragma unroll
        for (int k = 0; k < 6; k++) L.err[id * 6ull + k] = e[k];
        L.chi2[id] = chi2; L.rho1[id] = rho1;

        // Ji = [[-Ra, 2 Ra [tb]x], [0, -((wb I - [vb]x)(wa I + [va]x) - vb va^T)]], a = conj(mq), b = qb, times the sign that made w >= 0 -- which
        // is the sign of the product a b against qe;  Jj = [[Re, 0], [0, we I + [ve]x]]
        double Ji[36], Jj[36];
#pragma unroll
        for (int k = 0; k < 36; k++) { Ji[k] = 0.0; Jj[k] = 0.0; }
        double Rm[9], Re[9];
        q_to_R(mq, Rm);
        q_to_R(qe, Re);
        const double X[9] = {0.0, -tb[2], tb[1], tb[2], 0.0, -tb[0], -tb[1], tb[0], 0.0};
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                Ji[r * 6 + c] = -Rm[c * 3 + r];
                Ji[r * 6 + 3 + c] = 2.0 * ((Rm[r] * X[c] + Rm[3 + r] * X[3 + c]) + Rm[6 + r] * X[6 + c]);
                Jj[r * 6 + c] = Re[r * 3 + c];
            }
        }
        const double a[4] = {-mq[0], -mq[1], -mq[2], mq[3]};
        double raw[4];
        q_mul(a, qb, raw);
        const double sgn = (((raw[0] * qe[0] + raw[1] * qe[1]) + raw[2] * qe[2]) + raw[3] * qe[3]) < 0 ? -1.0 : 1.0;
        const double A1[9] = {qb[3], qb[2], -qb[1], -qb[2], qb[3], qb[0], qb[1], -qb[0], qb[3]};   // wb I - [vb]x
        const double A2[9] = {a[3], -a[2], a[1], a[2], a[3], -a[0], -a[1], a[0], a[3]};            // wa I + [va]x
        const double U[9] = {qe[3], -qe[2], qe[1], qe[2], qe[3], -qe[0], -qe[1], qe[0], qe[3]};    // we I + [ve]x
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double l = ((A1[r * 3] * A2[c] + A1[r * 3 + 1] * A2[3 + c]) + A1[r * 3 + 2] * A2[6 + c]) - qb[r] * a[c];
                Ji[(3 + r) * 6 + 3 + c] = -sgn * l;
                Jj[(3 + r) * 6 + 3 + c] = U[r * 3 + c];
            }
        }
        double* o = L.Ji + id * 36ull;
#pragma unroll
        for (int k = 0; k < 36; k++) o[k] = Ji[k];
        o = L.Jj + id * 36ull;
#pragma unroll
        for (int k = 0; k < 36; k++) o[k] = Jj[k];
        // b = -J^T (rho' Omega) e
#pragma unroll
        for (int r = 0; r < 6; r++) {
            double si = 0.0, sj = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) { si += Ji[k * 6 + r] * (rho1 * We[k]); sj += Jj[k * 6 + r] * (rho1 * We[k]); }
            L.bi[id * 6ull + r] = -si; L.bj[id * 6ull + r] = -sj;
        }
        // T = (rho' Omega) Jj, then Hjj = Jj^T T, Hij = Ji^T T; T = (rho' Omega) Ji, Hii = Ji^T T
        double T[36];
#pragma unroll
        for (int r = 0; r < 6; r++) {
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) s += (rho1 * ed.info[r * 6 + k]) * Jj[k * 6 + c];
                T[r * 6 + c] = s;
            }
        }
        atb_store(Jj, T, L.Hjj + id * 36ull);
        atb_store(Ji, T, L.Hij + id * 36ull);
#pragma unroll
        for (int r = 0; r < 6; r++) {
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) s += (rho1 * ed.info[r * 6 + k]) * Ji[k * 6 + c];
                T[r * 6 + c] = s;
            }
        }
        atb_store(Ji, T, L.Hii + id * 36ull);
    }
}

// one lane per prior (grid-stride): e (three of the id's six slots), chi2, rho', and into the id's Hii / bi slots the 6 x 6 J^T (rho' Omega) J and
// -J^T (rho' Omega) e of its node.  J is 3 x 6 with one non-zero 3 x 3 half (PLANE: the rotation half and a translation row), so the product is
// taken on 3 x 3 pieces and the 6 x 6 is never held in registers
__global__ void __launch_bounds__(kEdgeThreads) graph_linearize_prior(const PriorDev* __restrict__ priors, uint32_t n, const double* __restrict__ nt,
                                                                      const double* __restrict__ nq, const LmState* __restrict__ st, int tag, LinBuf L) {
    if (!wanted(st, tag)) return;
    for (uint32_t k0 = blockIdx.x * kEdgeThreads + threadIdx.x; k0 < n; k0 += gridDim.x * kEdgeThreads) {
        const PriorDev& pr = priors[k0];
        if (!pr.live) continue;  // (graph_linearize has zeroed the id's error, chi2 and rho')
        const uint64_t id = (uint64_t)pr.id;
        double t[3], q[4], m[4], pl[4], e[3], A[9], nl[3], u[3], We[3], sgn = 1.0;
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = nt[pr.node * 3ull + k];
#pragma unroll
        for (int k = 0; k < 4; k++) { q[k] = nq[pr.node * 4ull + k]; m[k] = pr.m[k]; pl[k] = pr.plane[k]; }
        prior_eval(pr.type, t, q, m, pl, e, A, nl, u, &sgn);
        const double chi2 = prior_chi2(e, pr.info, We);
        double rho, rho1;
        robustify(chi2, pr.kernel, pr.delta, &rho, &rho1);
#pragma unroll
        for (int k = 0; k < 3; k++) { L.err[id * 6 + k] = e[k]; L.err[id * 6 + 3 + k] = 0.0; }
        L.chi2[id] = chi2; L.rho1[id] = rho1;
        // J = [Jt | Jr], each 3 x 3
        double Jt[9], Jr[9];
#pragma unroll
        for (int k = 0; k < 9; k++) { Jt[k] = 0.0; Jr[k] = 0.0; }
        if (pr.type == LIO_GRAPH_PRIOR_XYZ) {
            q_to_R(q, Jt);
        } else if (pr.type == LIO_GRAPH_PRIOR_QUAT) {  // s (w I + [v]x)
            Jr[0] = sgn * q[3];  Jr[1] = -sgn * q[2]; Jr[2] = sgn * q[1];
            Jr[3] = sgn * q[2];  Jr[4] = sgn * q[3];  Jr[5] = -sgn * q[0];
            Jr[6] = -sgn * q[1]; Jr[7] = sgn * q[0];  Jr[8] = sgn * q[3];
        } else {
            // D = 2 A^T [n_l]x; rows 0 and 1 of Jr are g0 D and g1 D; they stay zero when r^2 = 0
            const double X[9] = {0.0, -nl[2], nl[1], nl[2], 0.0, -nl[0], -nl[1], nl[0], 0.0};
            const double r2 = u[0] * u[0] + u[1] * u[1];
            if (r2 > 0) {
                const double r = sqrt(r2);
                const double g0[3] = {-u[1] / r2, u[0] / r2, 0.0};
                const double g1[3] = {-u[0] * u[2] / r, -u[1] * u[2] / r, r};
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    double D[3];
#pragma unroll
                    for (int a = 0; a < 3; a++) D[a] = 2.0 * ((A[a] * X[c] + A[3 + a] * X[3 + c]) + A[6 + a] * X[6 + c]);
                    Jr[c] = (g0[0] * D[0] + g0[1] * D[1]) + g0[2] * D[2];
                    Jr[3 + c] = (g1[0] * D[0] + g1[1] * D[1]) + g1[2] * D[2];
                }
            }
            Jt[6] = -nl[0]; Jt[7] = -nl[1]; Jt[8] = -nl[2];
        }
        // b = -J^T (rho' Omega e);  H = J^T (rho' Omega) J by halves
        double* bo = L.bi + id * 6;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            bo[c] = -((Jt[c] * (rho1 * We[0]) + Jt[3 + c] * (rho1 * We[1])) + Jt[6 + c] * (rho1 * We[2]));
            bo[3 + c] = -((Jr[c] * (rho1 * We[0]) + Jr[3 + c] * (rho1 * We[1])) + Jr[6 + c] * (rho1 * We[2]));
        }
        double Tt[9], Tr[9];  // (rho' Omega) Jt, (rho' Omega) Jr
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                Tt[r * 3 + c] = ((rho1 * pr.info[r * 3]) * Jt[c] + (rho1 * pr.info[r * 3 + 1]) * Jt[3 + c]) + (rho1 * pr.info[r * 3 + 2]) * Jt[6 + c];
                Tr[r * 3 + c] = ((rho1 * pr.info[r * 3]) * Jr[c] + (rho1 * pr.info[r * 3 + 1]) * Jr[3 + c]) + (rho1 * pr.info[r * 3 + 2]) * Jr[6 + c];
            }
        }
        double* Ho = L.Hii + id * 36;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                Ho[r * 6 + c] = (Jt[r] * Tt[c] + Jt[3 + r] * Tt[3 + c]) + Jt[6 + r] * Tt[6 + c];
                Ho[r * 6 + 3 + c] = (Jt[r] * Tr[c] + Jt[3 + r] * Tr[3 + c]) + Jt[6 + r] * Tr[6 + c];
                Ho[(3 + r) * 6 + c] = (Jr[r] * Tt[c] + Jr[3 + r] * Tt[3 + c]) + Jr[6 + r] * Tt[6 + c];
                Ho[(3 + r) * 6 + 3 + c] = (Jr[r] * Tr[c] + Jr[3 + r] * Tr[3 + c]) + Jr[6 + r] * Tr[6 + c];
            }
        }
    }
}

// the moment stage (include/lio_hip.h, "moment"): one lane per prior (grid-stride), after graph_linearize_prior on the same stream.  A live XYZ
// prior is an EdgeSE3GNSS on its node and the shared moment m: e = t - (z + R m), J = [R | 2 R [m]x], J_m = -R.  The node's 6 x 6 and b overwrite
// what graph_linearize_prior left in the id's Hii / bi slots; the coupling block J^T (rho' Omega) J_m, J_m^T (rho' Omega) J_m and
// -J_m^T (rho' Omega) e go to the prior's record in mlin.  Priors of the other types, and dead ones, are left as they are
__global__ void __launch_bounds__(kEdgeThreads) graph_linearize_moment(const PriorDev* __restrict__ priors, uint32_t n, const double* __restrict__ nt,
                                                                       const double* __restrict__ nq, const LmState* __restrict__ st, int tag, LinBuf L,
                                                                       const double* __restrict__ mom, double* __restrict__ mlin) {
    if (!wanted(st, tag)) return;
    for (uint32_t k0 = blockIdx.x * kEdgeThreads + threadIdx.x; k0 < n; k0 += gridDim.x * kEdgeThreads) {
        const PriorDev& pr = priors[k0];
        if (!pr.live || pr.type != LIO_GRAPH_PRIOR_XYZ) continue;
        const uint64_t id = (uint64_t)pr.id;
        double t[3], q[4], z[3], m[3], e[3], We[3], Jt[9], Jr[9], Jm[9];
#pragma unroll
        for (int k = 0; k < 3; k++) { t[k] = nt[pr.node * 3ull + k]; z[k] = pr.m[k]; m[k] = mom[kMomM + k]; }
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = nq[pr.node * 4ull + k];
        q_to_R(q, Jt);
        moment_eval(t, Jt, z, m, e);
        const double chi2 = prior_chi2(e, pr.info, We);
        double rho, rho1;
        robustify(chi2, pr.kernel, pr.delta, &rho, &rho1);
#pragma unroll
        for (int k = 0; k < 3; k++) { L.err[id * 6 + k] = e[k]; L.err[id * 6 + 3 + k] = 0.0; }
        L.chi2[id] = chi2; L.rho1[id] = rho1;
        const double X[9] = {0.0, -m[2], m[1], m[2], 0.0, -m[0], -m[1], m[0], 0.0};
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                Jr[r * 3 + c] = 2.0 * ((Jt[r * 3] * X[c] + Jt[r * 3 + 1] * X[3 + c]) + Jt[r * 3 + 2] * X[6 + c]);
                Jm[r * 3 + c] = -Jt[r * 3 + c];
            }
        }
        double* bo = L.bi + id * 6;
        double* mo = mlin + k0 * (uint64_t)kMlinDoubles;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            bo[c] = -((Jt[c] * (rho1 * We[0]) + Jt[3 + c] * (rho1 * We[1])) + Jt[6 + c] * (rho1 * We[2]));
            bo[3 + c] = -((Jr[c] * (rho1 * We[0]) + Jr[3 + c] * (rho1 * We[1])) + Jr[6 + c] * (rho1 * We[2]));
            mo[kMlinBm + c] = -((Jm[c] * (rho1 * We[0]) + Jm[3 + c] * (rho1 * We[1])) + Jm[6 + c] * (rho1 * We[2]));
        }
        double Tt[9], Tr[9], Tm[9];  // (rho' Omega) Jt, (rho' Omega) Jr, (rho' Omega) Jm
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                Tt[r * 3 + c] = ((rho1 * pr.info[r * 3]) * Jt[c] + (rho1 * pr.info[r * 3 + 1]) * Jt[3 + c]) + (rho1 * pr.info[r * 3 + 2]) * Jt[6 + c];
                Tr[r * 3 + c] = ((rho1 * pr.info[r * 3]) * Jr[c] + (rho1 * pr.info[r * 3 + 1]) * Jr[3 + c]) + (rho1 * pr.info[r * 3 + 2]) * Jr[6 + c];
                Tm[r * 3 + c] = ((rho1 * pr.info[r * 3]) * Jm[c] + (rho1 * pr.info[r * 3 + 1]) * Jm[3 + c]) + (rho1 * pr.info[r * 3 + 2]) * Jm[6 + c];
            }
        }
        double* Ho = L.Hii + id * 36;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                Ho[r * 6 + c] = (Jt[r] * Tt[c] + Jt[3 + r] * Tt[3 + c]) + Jt[6 + r] * Tt[6 + c];
                Ho[r * 6 + 3 + c] = (Jt[r] * Tr[c] + Jt[3 + r] * Tr[3 + c]) + Jt[6 + r] * Tr[6 + c];
                Ho[(3 + r) * 6 + c] = (Jr[r] * Tt[c] + Jr[3 + r] * Tt[3 + c]) + Jr[6 + r] * Tt[6 + c];
                Ho[(3 + r) * 6 + 3 + c] = (Jr[r] * Tr[c] + Jr[3 + r] * Tr[3 + c]) + Jr[6 + r] * Tr[6 + c];
                mo[kMlinHpm + r * 3 + c] = (Jt[r] * Tm[c] + Jt[3 + r] * Tm[3 + c]) + Jt[6 + r] * Tm[6 + c];
                mo[kMlinHpm + (3 + r) * 3 + c] = (Jr[r] * Tm[c] + Jr[3 + r] * Tm[3 + c]) + Jr[6 + r] * Tm[6 + c];
                mo[kMlinHmm + r * 3 + c] = (Jm[r] * Tm[c] + Jm[3 + r] * Tm[3 + c]) + Jm[6 + r] * Tm[6 + c];
            }
        }
    }
}

// the border of the moment stage: Hpm [Na x 18] = per active node the sum of its moment edges' coupling blocks, Hmm [9] and bm [3] = the sums over
// all moment edges plus the moment's own prior (Omega_m, -Omega_m m).  One lane per entry; mptr / mlist hold prior indices in rising edge id (a
// prior's index rises with its id), all [n_all] the moment edges of the whole graph, those on fixed nodes included: no atomics
__global__ void __launch_bounds__(256) graph_assemble_border(const LmState* __restrict__ st, int tag, uint32_t Na, const uint32_t* __restrict__ mptr,
                                                             const uint32_t* __restrict__ mlist, const uint32_t* __restrict__ all, uint32_t n_all,
                                                             const double* __restrict__ mlin, const double* __restrict__ mom, double* __restrict__ Hpm,
                                                             double* __restrict__ Hmm, double* __restrict__ bm) {
    if (!wanted(st, tag)) return;
    const uint64_t np = 18ull * Na;
    for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < np + 12; g += gridDim.x * 256ull) {
        double s = 0.0;
        if (g < np) {
            const uint32_t a = (uint32_t)(g / 18), k = (uint32_t)(g % 18);
            for (uint32_t i = mptr[a]; i < mptr[a + 1]; i++) s += mlin[mlist[i] * (uint64_t)kMlinDoubles + kMlinHpm + k];
            Hpm[g] = s;
        } else if (g < np + 9) {
            const uint32_t k = (uint32_t)(g - np);
            for (uint32_t i = 0; i < n_all; i++) s += mlin[all[i] * (uint64_t)kMlinDoubles + kMlinHmm + k];
            Hmm[k] = s + mom[kMomInfo + k];
        } else {
            const uint32_t k = (uint32_t)(g - np - 9);
            for (uint32_t i = 0; i < n_all; i++) s += mlin[all[i] * (uint64_t)kMlinDoubles + kMlinBm + k];
            const double* W = mom + kMomInfo + k * 3;
            bm[k] = s - ((W[0] * mom[kMomM] + W[1] * mom[kMomM + 1]) + W[2] * mom[kMomM + 2]);
        }
    }
}

// Hd [Na x 36], Ho [P x 36], b [6 Na]: item = (block, entry); the lists hold (edge << 1 | flag) in rising edge id
__global__ void __launch_bounds__(256) graph_assemble(const LmState* __restrict__ st, int tag, uint32_t Na, uint32_t P, const uint32_t* __restrict__ dptr,
                                                      const uint32_t* __restrict__ dlist, const uint32_t* __restrict__ pptr, const uint32_t* __restrict__ plist,
                                                      LinBuf L, double* __restrict__ Hd, double* __restrict__ Ho, double* __restrict__ b) {
    if (!wanted(st, tag)) return;
    const uint64_t nd = 36ull * Na, np = 36ull * P, nb = 6ull * Na;
    for (uint64_t g = blockIdx.x * 256ull + threadIdx.x; g < nd + np + nb; g += gridDim.x * 256ull) {
        double s = 0.0;
        if (g < nd) {
            const uint32_t a = (uint32_t)(g / 36), k = (uint32_t)(g % 36);
            for (uint32_t i = dptr[a]; i < dptr[a + 1]; i++) { const uint32_t w = dlist[i]; s += ((w & 1u) ? L.Hjj : L.Hii)[(w >> 1) * 36ull + k]; }
            Hd[g] = s;
        } else if (g < nd + np) {
            const uint64_t h = g - nd;
            const uint32_t p = (uint32_t)(h / 36), k = (uint32_t)(h % 36), kt = (k % 6) * 6 + k / 6;
            for (uint32_t i = pptr[p]; i < pptr[p + 1]; i++) { const uint32_t w = plist[i]; s += L.Hij[(w >> 1) * 36ull + ((w & 1u) ? kt : k)]; }
            Ho[h] = s;
        } else {
            const uint64_t h = g - nd - np;
            const uint32_t a = (uint32_t)(h / 6), k = (uint32_t)(h % 6);
            for (uint32_t i = dptr[a]; i < dptr[a + 1]; i++) { const uint32_t w = dlist[i]; s += ((w & 1u) ? L.bj : L.bi)[(w >> 1) * 6ull + k]; }
            b[h] = s;
        }
    }
}

// the sum of one value per lane of the workgroup, the same bits in every lane: xor butterflies inside a wave (a + b = b + a), then the waves in order
__device__ inline double block_sum(double v, double* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) s += sh[w];
    return s;
}
__device__ inline double block_max(double v, double* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) s = fmax(s, sh[w]);
    return s;
}

// inverse of the SPD block (lower triangle of A + lambda I, packed) in place: Cholesky, the factor's inverse, Li^T Li; false: not positive definite
__device__ inline bool inv6_spd(const double* __restrict__ A, double lambda, double* __restrict__ out) {
#define IX(i, j) ((i) * ((i) + 1) / 2 + (j))
    double a[21];
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) a[IX(i, j)] = A[i * 6 + j] + (i == j ? lambda : 0.0);
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double s = a[IX(j, j)];
#pragma unroll
        for (int k = 0; k < j; k++) s -= a[IX(j, k)] * a[IX(j, k)];
        if (!(s > 0)) { ok = false; s = 1.0; }
        const double d = sqrt(s);
        a[IX(j, j)] = d;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double t = a[IX(i, j)];
#pragma unroll
            for (int k = 0; k < j; k++) t -= a[IX(i, k)] * a[IX(j, k)];
            a[IX(i, j)] = t / d;
        }
    }
#pragma unroll
    for (int j = 0; j < 6; j++) {
        a[IX(j, j)] = 1.0 / a[IX(j, j)];
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double t = 0.0;
#pragma unroll
            for (int k = j; k < i; k++) t -= a[IX(i, k)] * a[IX(k, j)];
            a[IX(i, j)] = t / a[IX(i, i)];
        }
    }
#pragma unroll
    for (int r = 0; r < 6; r++) {
#pragma unroll
        for (int c = 0; c <= r; c++) {
            double s = 0.0;
#pragma unroll
            for (int k = r; k < 6; k++) s += a[IX(k, r)] * a[IX(k, c)];
            out[r * 6 + c] = s;
            out[c * 6 + r] = s;
        }
    }
#undef IX
    return ok;
}

// inverse of the damped SPD 3 x 3 (row-major) by Cholesky, as inv6_spd; false: not positive definite
__device__ inline bool inv3_spd(const double* __restrict__ A, double lambda, double* __restrict__ out) {
    bool ok = true;
    double s = A[0] + lambda;
    if (!(s > 0)) { ok = false; s = 1.0; }
    const double l00 = sqrt(s), l10 = A[3] / l00, l20 = A[6] / l00;
    s = (A[4] + lambda) - l10 * l10;
    if (!(s > 0)) { ok = false; s = 1.0; }
    const double l11 = sqrt(s), l21 = (A[7] - l20 * l10) / l11;
    s = ((A[8] + lambda) - l20 * l20) - l21 * l21;
    if (!(s > 0)) { ok = false; s = 1.0; }
    const double l22 = sqrt(s);
    // the factor's inverse (lower), then Li^T Li
    const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
    const double i10 = -(l10 * i00) / l11, i21 = -(l21 * i11) / l22, i20 = -(l20 * i00 + l21 * i10) / l22;
    out[0] = (i00 * i00 + i10 * i10) + i20 * i20;
    out[1] = out[3] = i10 * i11 + i20 * i21;
    out[2] = out[6] = i20 * i22;
    out[4] = i11 * i11 + i21 * i21;
    out[5] = out[7] = i21 * i22;
    out[8] = i22 * i22;
    return ok;
}

// the border of the moment stage as graph_solve sees it: three more unknowns behind the 6 Na of the nodes
struct BorderArgs {
    const double *Hpm, *Hmm, *bm;  // [Na x 18] coupling blocks (6 x 3 each), the border's 3 x 3, its 3 of b
    double* Minv3;                 // [9] the inverse of the damped 3 x 3
};

// one trial's (H + lambda I) d = b by preconditioned conjugate gradients, one workgroup.  vec: x, r, z, p, Ap of n each, n = 6 Na, or 6 Na + 3 with
// the border (kBorder): rows 6 Na .. 6 Na + 2 are the moment's.  The preconditioner then has the damped 3 x 3's inverse as one more block, a node
// row of the product adds Hpm[a] p_m, and a border row is Hmm p_m + lambda p_m + sum_a Hpm[a]^T p_a, the sum folded by block_sum.  Without the
// border every `kBorder &&` branch is compiled away and the text is the solve as it always was
template <bool kBorder>
__device__ __forceinline__ void solve_body(LmState* __restrict__ st, int tag, uint32_t Na, const double* __restrict__ Hd, const double* __restrict__ Ho,
                                           const double* __restrict__ b, const uint32_t* __restrict__ rptr, const uint32_t* __restrict__ rcol,
                                           const uint32_t* __restrict__ rblk, double* __restrict__ Minv, double* __restrict__ vec, double cg_epsilon,
                                           int cg_max_iterations, const BorderArgs B) {
    if (!wanted(st, tag)) return;
    __shared__ double sh[kSolveThreads / 64];
    const uint32_t n6 = 6u * Na, n = kBorder ? n6 + 3u : n6, tid = threadIdx.x;
    double* x = vec;
    double* r = vec + n;
    double* z = vec + 2ull * n;
    double* p = vec + 3ull * n;
    double* Ap = vec + 4ull * n;
    double lambda = st->lambda;
    const int need_init = st->need_lambda_init;
    const int cg_total0 = st->cg_total;
    if (need_init) {  // computeLambdaInit: tau max |diag H|
        double m = 0.0;
        for (uint32_t i = tid; i < n; i += kSolveThreads) m = fmax(m, fabs(kBorder && i >= n6 ? B.Hmm[(i - n6) * 4] : Hd[(i / 6) * 36ull + (i % 6) * 7]));
        lambda = 1e-5 * block_max(m, sh);
    }
    double okf = 1.0;
    for (uint32_t a = tid; a < Na; a += kSolveThreads)
        if (!inv6_spd(Hd + a * 36ull, lambda, Minv + a * 36ull)) okf = 0.0;
    if (kBorder && tid == kSolveThreads - 1)
        if (!inv3_spd(B.Hmm, lambda, B.Minv3)) okf = 0.0;
    double bb = 0.0;
    for (uint32_t i = tid; i < n; i += kSolveThreads) { const double v = kBorder && i >= n6 ? B.bm[i - n6] : b[i]; bb += v * v; x[i] = 0.0; r[i] = v; }
    bb = block_sum(bb, sh);  // (its barriers also publish Minv and r)
    const double bad = block_sum(1.0 - okf, sh);
    double rz = 0.0;
    for (uint32_t i = tid; i < n; i += kSolveThreads) {
        double s = 0.0;
        if (kBorder && i >= n6) {
            const uint32_t k = i - n6;
            s = (B.Minv3[k * 3] * r[n6] + B.Minv3[k * 3 + 1] * r[n6 + 1]) + B.Minv3[k * 3 + 2] * r[n6 + 2];
        } else {
            const uint32_t a = i / 6, k = i % 6;
#pragma unroll
            for (int c = 0; c < 6; c++) s += Minv[a * 36ull + k * 6 + c] * r[a * 6ull + c];
        }
        z[i] = s; p[i] = s;
        rz += r[i] * s;
    }
    rz = block_sum(rz, sh);
    const double tol2 = (cg_epsilon * cg_epsilon) * bb;
    double rr = bb;
    int it = 0;
    bool ok = bad == 0.0 && bb - bb == 0.0;
    while (ok && it < cg_max_iterations && rr > tol2) {
        double pAp = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;  // c: this lane's share of sum_a Hpm[a]^T p_a
        for (uint32_t i = tid; i < n6; i += kSolveThreads) {
            const uint32_t a = i / 6, k = i % 6;
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < 6; c++) s += Hd[a * 36ull + k * 6 + c] * p[a * 6ull + c];
            s += lambda * p[i];
            for (uint32_t e = rptr[a]; e < rptr[a + 1]; e++) {
                const uint32_t w = rblk[e];
                const double* Bk = Ho + (w & 0x7FFFFFFFu) * 36ull;
                const double* pc = p + rcol[e] * 6ull;
                if (w >> 31) {
#pragma unroll
                    for (int c = 0; c < 6; c++) s += Bk[c * 6 + k] * pc[c];
                } else {
#pragma unroll
                    for (int c = 0; c < 6; c++) s += Bk[k * 6 + c] * pc[c];
                }
            }
            if (kBorder) {
                const double* C = B.Hpm + a * 18ull + k * 3;
                s += (C[0] * p[n6] + C[1] * p[n6 + 1]) + C[2] * p[n6 + 2];
                c0 += C[0] * p[i]; c1 += C[1] * p[i]; c2 += C[2] * p[i];
            }
            Ap[i] = s;
            pAp += p[i] * s;
        }
        if (kBorder) {
            c0 = block_sum(c0, sh); c1 = block_sum(c1, sh); c2 = block_sum(c2, sh);
            if (tid < 3) {  // the border's rows
                const uint32_t i = n6 + tid;
                const double* H = B.Hmm + tid * 3;
                const double s = (((H[0] * p[n6] + H[1] * p[n6 + 1]) + H[2] * p[n6 + 2]) + lambda * p[i]) + (tid == 0 ? c0 : tid == 1 ? c1 : c2);
                Ap[i] = s;
                pAp += p[i] * s;
            }
        }
        pAp = block_sum(pAp, sh);
        if (!(pAp > 0)) break;  // (the same bits in every lane: the whole workgroup leaves)
        const double alpha = rz / pAp;
        double rr2 = 0.0;
        for (uint32_t i = tid; i < n; i += kSolveThreads) {
            x[i] += alpha * p[i];
            const double v = r[i] - alpha * Ap[i];
            r[i] = v;
            rr2 += v * v;
        }
        rr = block_sum(rr2, sh);
        it++;
        if (!(rr > tol2)) break;
        double rz2 = 0.0;
        for (uint32_t i = tid; i < n; i += kSolveThreads) {
            double s = 0.0;
            if (kBorder && i >= n6) {
                const uint32_t k = i - n6;
                s = (B.Minv3[k * 3] * r[n6] + B.Minv3[k * 3 + 1] * r[n6 + 1]) + B.Minv3[k * 3 + 2] * r[n6 + 2];
            } else {
                const uint32_t a = i / 6, k = i % 6;
#pragma unroll
                for (int c = 0; c < 6; c++) s += Minv[a * 36ull + k * 6 + c] * r[a * 6ull + c];
            }
            z[i] = s;
            rz2 += r[i] * s;
        }
        rz2 = block_sum(rz2, sh);
        const double beta = rz2 / rz;
        rz = rz2;
        for (uint32_t i = tid; i < n; i += kSolveThreads) p[i] = z[i] + beta * p[i];
        __syncthreads();
    }
    // computeScale: d^T (lambda d + b)
    double sc = 0.0;
    for (uint32_t i = tid; i < n; i += kSolveThreads) sc += x[i] * (lambda * x[i] + (kBorder && i >= n6 ? B.bm[i - n6] : b[i]));
    sc = block_sum(sc, sh);
    if (tid == 0) {
        st->lambda = lambda;
        if (need_init) { st->nu = 2.0; st->need_lambda_init = 0; }
        st->scale = sc + 1e-3;
        st->solve_ok = ok ? 1 : 0;
        st->cg_iterations = it;
        st->cg_total = cg_total0 + it;
        st->cg_relres = bb > 0 ? sqrt(rr / bb) : 0.0;
    }
}
__global__ void __launch_bounds__(kSolveThreads) graph_solve(LmState* __restrict__ st, int tag, uint32_t Na, const double* __restrict__ Hd, const double* __restrict__ Ho,
                                                             const double* __restrict__ b, const uint32_t* __restrict__ rptr, const uint32_t* __restrict__ rcol,
                                                             const uint32_t* __restrict__ rblk, double* __restrict__ Minv, double* __restrict__ vec,
                                                             double cg_epsilon, int cg_max_iterations) {
    solve_body<false>(st, tag, Na, Hd, Ho, b, rptr, rcol, rblk, Minv, vec, cg_epsilon, cg_max_iterations, BorderArgs{nullptr, nullptr, nullptr, nullptr});
}
// the same solve over the bordered system of the moment stage
__global__ void __launch_bounds__(kSolveThreads) graph_solve_border(LmState* __restrict__ st, int tag, uint32_t Na, const double* __restrict__ Hd,
                                                                    const double* __restrict__ Ho, const double* __restrict__ b, const uint32_t* __restrict__ rptr,
                                                                    const uint32_t* __restrict__ rcol, const uint32_t* __restrict__ rblk, double* __restrict__ Minv,
                                                                    double* __restrict__ vec, double cg_epsilon, int cg_max_iterations, BorderArgs B) {
    solve_body<true>(st, tag, Na, Hd, Ho, b, rptr, rcol, rblk, Minv, vec, cg_epsilon, cg_max_iterations, B);
}

// backup + update of the active nodes
__global__ void __launch_bounds__(256) graph_update(const LmState* __restrict__ st, int tag, uint32_t Na, const uint32_t* __restrict__ act, const double* __restrict__ d,
                                                    double* __restrict__ nt, double* __restrict__ nq, double* __restrict__ bak) {
    if (!wanted(st, tag)) return;
    const uint32_t a = blockIdx.x * 256u + threadIdx.x;
    if (a >= Na) return;
    const uint32_t n = act[a];
    double t[3], q[4], dd[6];
#pragma unroll
    for (int k = 0; k < 3; k++) { t[k] = nt[n * 3ull + k]; bak[a * 7ull + k] = t[k]; }
#pragma unroll
    for (int k = 0; k < 4; k++) { q[k] = nq[n * 4ull + k]; bak[a * 7ull + 3 + k] = q[k]; }
#pragma unroll
    for (int k = 0; k < 6; k++) dd[k] = d[a * 6ull + k];
    apply_delta(t, q, dd);
#pragma unroll
    for (int k = 0; k < 3; k++) nt[n * 3ull + k] = t[k];
#pragma unroll
    for (int k = 0; k < 4; k++) nq[n * 4ull + k] = q[k];
}

// the moment stage's update, beside graph_update: backup + m <- m + d_m (VertexPointXYZ adds); d_m = the three entries behind the nodes' 6 Na
__global__ void __launch_bounds__(64) graph_update_moment(const LmState* __restrict__ st, int tag, const double* __restrict__ dm, double* __restrict__ mom) {
    if (!wanted(st, tag)) return;
    if (blockIdx.x == 0 && threadIdx.x < 3) {
        const double m = mom[kMomM + threadIdx.x];
        mom[kMomBak + threadIdx.x] = m;
        mom[kMomM + threadIdx.x] = m + dm[threadIdx.x];
    }
}

// rho of every edge; one partial per 256 consecutive edge ids.  kPriors: an id may be a prior's placeholder, whose rho is taken from the prior;
// kMoment: the stage is open and a live XYZ prior is a moment edge at the current m
template <bool kPriors, bool kMoment>
__device__ __forceinline__ void chi2_body(const LmState* __restrict__ st, int tag, const EdgeDev* __restrict__ edges, uint32_t E, const PriorDev* __restrict__ priors,
                                          const double* __restrict__ nt, const double* __restrict__ nq, double* __restrict__ partial, const double* __restrict__ mom) {
    if (!wanted(st, tag)) return;
    __shared__ double sh[kEdgeThreads / 64];
    const uint32_t id = blockIdx.x * kEdgeThreads + threadIdx.x;
    double rho = 0.0;
    if (kPriors && id < E && edges[id].live == kPriorSlot) {
        const PriorDev& pr = priors[edges[id].from];
        if (kMoment && pr.live && pr.type == LIO_GRAPH_PRIOR_XYZ) rho = moment_rho(pr, nt, nq, mom);
        else if (pr.live) rho = prior_rho(pr, nt, nq);
    } else if (id < E && edges[id].live) {
        const EdgeDev& ed = edges[id];
        double ti[3], qi[4], tj[3], qj[4], mt[3], mq[4];
#pragma unroll
        for (int k = 0; k < 3; k++) { ti[k] = nt[ed.from * 3ull + k]; tj[k] = nt[ed.to * 3ull + k]; mt[k] = ed.mt[k]; }
#pragma unroll
        for (int k = 0; k < 4; k++) { qi[k] = nq[ed.from * 4ull + k]; qj[k] = nq[ed.to * 4ull + k]; mq[k] = ed.mq[k]; }
        double e[6], tb[3], qb[4], qe[4], We[6], rho1;
        edge_eval(ti, qi, tj, qj, mt, mq, e, tb, qb, qe);
        robustify(edge_chi2(e, ed.info, We), ed.kernel, ed.delta, &rho, &rho1);
    }
    const double s = block_sum(rho, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
template <bool kPriors>
__global__ void __launch_bounds__(kEdgeThreads) graph_chi2(const LmState* __restrict__ st, int tag, const EdgeDev* __restrict__ edges, uint32_t E,
                                                           const PriorDev* __restrict__ priors, const double* __restrict__ nt, const double* __restrict__ nq,
                                                           double* __restrict__ partial) {
    chi2_body<kPriors, false>(st, tag, edges, E, priors, nt, nq, partial, nullptr);
}
__global__ void __launch_bounds__(kEdgeThreads) graph_chi2_moment(const LmState* __restrict__ st, int tag, const EdgeDev* __restrict__ edges, uint32_t E,
                                                                  const PriorDev* __restrict__ priors, const double* __restrict__ nt, const double* __restrict__ nq,
                                                                  double* __restrict__ partial, const double* __restrict__ mom) {
    chi2_body<true, true>(st, tag, edges, E, priors, nt, nq, partial, mom);
}

// one workgroup: the new chi2 (partials in order), the LM bookkeeping of OptimizationAlgorithmLevenberg::solve, the restore of a rejected trial.
// kMoment: the moment's own prior adds m^T Omega m after the partials, and a rejected trial restores m with the poses
template <bool kMoment>
__device__ __forceinline__ void decide_body(LmState* __restrict__ st, int tag, const double* __restrict__ partial, uint32_t nb, uint32_t Na,
                                            const uint32_t* __restrict__ act, const double* __restrict__ bak, double* __restrict__ nt, double* __restrict__ nq,
                                            int max_iterations, double chi2_rel_stop, double* __restrict__ mom) {
    __shared__ int s_go, s_accept;
    if (threadIdx.x == 0) s_go = wanted(st, tag) ? 1 : 0;  // (lane 0 rewrites the state below: every wave takes lane 0's answer)
    __syncthreads();
    if (!s_go) return;
    if (threadIdx.x == 0) {
        double c = 0.0;
        for (uint32_t k = 0; k < nb; k++) c += partial[k];
        if (kMoment) c += moment_prior_chi2(mom + kMomM, mom + kMomInfo);
        if (!st->solve_ok) c = DBL_MAX;
        const double rho = (st->chi2 - c) / st->scale;
        const bool accept = rho > 0 && c - c == 0.0 && st->solve_ok;
        double lambda = st->lambda;
        bool rel = false;
        if (accept) {
            const double t = 2.0 * rho - 1.0;
            double alpha = 1.0 - t * t * t;
            alpha = fmin(alpha, 2.0 / 3.0);
            lambda *= fmax(1.0 / 3.0, alpha);
            st->nu = 2.0;
            rel = chi2_rel_stop > 0 && (st->chi2 - c) <= chi2_rel_stop * st->chi2;
            st->chi2 = c;
            st->accepted++;
        } else {
            lambda *= st->nu;
            st->nu *= 2.0;
        }
        const bool lam_ok = lambda - lambda == 0.0;
        st->lambda = lambda;
        st->chi2_new = c;
        st->rho = rho;
        const int trials = st->trials + 1;
        st->total_trials++;
        st->trials = trials;
        if (!(rho < 0 && trials < kMaxTrials && lam_ok)) {  // the iteration is decided
            const int done = st->iteration + 1;
            st->iteration = done;
            st->trials = 0;
            st->batch = tag + 1;
            if (!lam_ok) st->stop = LIO_GRAPH_STOP_LAMBDA;
            else if (trials == kMaxTrials) st->stop = LIO_GRAPH_STOP_TRIALS;
            else if (rho == 0) st->stop = LIO_GRAPH_STOP_RHO_ZERO;
            else if (rel) st->stop = LIO_GRAPH_STOP_CHI2_REL;
            else if (done >= max_iterations) st->stop = LIO_GRAPH_STOP_MAX_ITERATIONS;
        }
        s_accept = accept ? 1 : 0;
    }
    __syncthreads();
    if (s_accept) return;
    for (uint32_t a = threadIdx.x; a < Na; a += 256u) {
        const uint32_t n = act[a];
#pragma unroll
        for (int k = 0; k < 3; k++) nt[n * 3ull + k] = bak[a * 7ull + k];
#pragma unroll
        for (int k = 0; k < 4; k++) nq[n * 4ull + k] = bak[a * 7ull + 3 + k];
    }
    if (kMoment && threadIdx.x < 3) mom[kMomM + threadIdx.x] = mom[kMomBak + threadIdx.x];
}
__global__ void __launch_bounds__(256) graph_decide(LmState* __restrict__ st, int tag, const double* __restrict__ partial, uint32_t nb, uint32_t Na,
                                                    const uint32_t* __restrict__ act, const double* __restrict__ bak, double* __restrict__ nt, double* __restrict__ nq,
                                                    int max_iterations, double chi2_rel_stop) {
    decide_body<false>(st, tag, partial, nb, Na, act, bak, nt, nq, max_iterations, chi2_rel_stop, nullptr);
}
__global__ void __launch_bounds__(256) graph_decide_moment(LmState* __restrict__ st, int tag, const double* __restrict__ partial, uint32_t nb, uint32_t Na,
                                                           const uint32_t* __restrict__ act, const double* __restrict__ bak, double* __restrict__ nt,
                                                           double* __restrict__ nq, int max_iterations, double chi2_rel_stop, double* __restrict__ mom) {
    decide_body<true>(st, tag, partial, nb, Na, act, bak, nt, nq, max_iterations, chi2_rel_stop, mom);
}

}  // namespace graph
}  // namespace lio

using namespace lio;
using namespace lio::graph;

struct lio_graph {
    int device = 0;
    lio_graph_params par;
    hipStream_t st = nullptr;
    hipEvent_t ev[kEvents] = {};
    // host mirror of the topology; a prior has to = -1, and pslot = its index in priors (-1 for a binary edge)
    std::vector<int32_t> from, to, pslot;
    std::vector<uint8_t> live, fixed;
    std::vector<uint8_t> gone;  // per node: removed (lio_graph_remove_node); its slot, its device row and its id stay
    // host mirror of every binary edge as it was added (lio_graph_edge_records); a prior's id holds an empty record
    struct EdgeRec { double M[16], info[36], delta; int32_t kernel; };
    std::vector<EdgeRec> rec;
    std::vector<PriorDev> priors;  // host mirror of every prior ever added; the first n_dev_priors are on the device
    uint32_t n_dev_priors = 0, prior_cap = 0;
    PriorDev* d_priors = nullptr;
    // not yet on the device: nodes as 7 doubles, edges
    std::vector<double> pend_nodes;
    std::vector<EdgeDev> pend_edges;
    uint32_t n_dev_nodes = 0, n_dev_edges = 0, node_cap = 0, edge_cap = 0;
    double *d_t = nullptr, *d_q = nullptr;
    EdgeDev* d_edges = nullptr;
    double* d_lin = nullptr;
    LinBuf lin{};
    // topology on the device
    bool topo_dirty = true;
    uint32_t Na = 0, P = 0, n_live = 0, nnz = 0;
    std::vector<uint32_t> act;  // active index -> node
    uint32_t* d_topo = nullptr;
    uint64_t topo_cap = 0;
    uint32_t *d_act = nullptr, *d_dptr = nullptr, *d_dlist = nullptr, *d_pptr = nullptr, *d_plist = nullptr, *d_rptr = nullptr, *d_rcol = nullptr, *d_rblk = nullptr;
    double* d_sys = nullptr;  // Hd, Ho, b, Minv, vec (5), bak
    uint64_t sys_cap = 0;
    double *d_Hd = nullptr, *d_Ho = nullptr, *d_b = nullptr, *d_Minv = nullptr, *d_vec = nullptr, *d_bak = nullptr;
    double *d_partial = nullptr, *h_partial = nullptr;
    uint32_t partial_cap = 0;
    LmState *d_state = nullptr, *h_state = nullptr;
    lio_graph_report rep{};
    double t_lin = 0, t_asm = 0, t_solve = 0, t_update = 0;
    // the moment stage, between lio_graph_moment_begin and _end: every live XYZ prior is an edge to one shared 3-DoF vertex, a border on the system
    bool moment_open = false, border_stale = true;
    double moment_info[9] = {};
    double* d_mom = nullptr;     // kMomDoubles; kept from the first begin on
    double* d_border = nullptr;  // Hmm, bm, Minv3, Hpm [18 Na], vec [5 (6 Na + 3)], mlin [kMlinDoubles per prior]
    uint64_t border_cap = 0;
    double *d_Hmm = nullptr, *d_bm = nullptr, *d_Minv3 = nullptr, *d_Hpm = nullptr, *d_bvec = nullptr, *d_mlin = nullptr;
    uint32_t* d_btopo = nullptr;  // mptr [Na + 1], mlist, all
    uint64_t btopo_cap = 0;
    uint32_t *d_mptr = nullptr, *d_mlist = nullptr, *d_mall = nullptr, n_mall = 0;
};

namespace {

uint32_t num_nodes(const lio_graph* g) { return (uint32_t)g->fixed.size(); }
uint32_t num_edges(const lio_graph* g) { return (uint32_t)g->from.size(); }
bool node_ok(const lio_graph* g, int id) { return id >= 0 && (uint32_t)id < num_nodes(g) && !g->gone[id]; }  // a removed id is as unknown as one never handed out

template <typename T>
int grow_copy(T** p, uint64_t old_n, uint64_t new_cap, hipStream_t st) {
    T* q = nullptr;
    LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q), new_cap * sizeof(T)));
    if (*p && old_n) {
        hipError_t e = hipMemcpyAsync(q, *p, old_n * sizeof(T), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { hipFree(q); set_error("lio_graph: %s", hipGetErrorString(e)); return LIO_E_DEVICE; }
    }
    if (*p) hipFree(*p);
    *p = q;
    return LIO_OK;
}

void set_lin(lio_graph* g) {
    const uint64_t c = g->edge_cap;
    double* p = g->d_lin;
    LinBuf& L = g->lin;
    L.err = p; p += 6 * c;
    L.chi2 = p; p += c;
    L.rho1 = p; p += c;
    L.Ji = p; p += 36 * c;
    L.Jj = p; p += 36 * c;
    L.Hii = p; p += 36 * c;
    L.Hij = p; p += 36 * c;
    L.Hjj = p; p += 36 * c;
    L.bi = p; p += 6 * c;
    L.bj = p;
}
constexpr uint64_t kLinPerEdge = 6 + 1 + 1 + 36 * 5 + 6 + 6;

// pending nodes and edges to the device
int flush(lio_graph* g) {
    const uint32_t N = num_nodes(g), E = num_edges(g);
    if (N > g->n_dev_nodes) {
        if (N > g->node_cap) {
            uint32_t c = g->node_cap ? g->node_cap : 1024;
            while (c < N) c *= 2;
            int rc = grow_copy(&g->d_t, 3ull * g->n_dev_nodes, 3ull * c, g->st);
            if (rc != LIO_OK) return rc;
            rc = grow_copy(&g->d_q, 4ull * g->n_dev_nodes, 4ull * c, g->st);
            if (rc != LIO_OK) return rc;
            g->node_cap = c;
        }
        const uint32_t k = N - g->n_dev_nodes;
        std::vector<double> t(3ull * k), q(4ull * k);
        for (uint32_t i = 0; i < k; i++) {
            for (int j = 0; j < 3; j++) t[3ull * i + j] = g->pend_nodes[7ull * i + j];
            for (int j = 0; j < 4; j++) q[4ull * i + j] = g->pend_nodes[7ull * i + 3 + j];
        }
        LIO_HIP_TRY(hipMemcpy(g->d_t + 3ull * g->n_dev_nodes, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
        LIO_HIP_TRY(hipMemcpy(g->d_q + 4ull * g->n_dev_nodes, q.data(), q.size() * sizeof(double), hipMemcpyHostToDevice));
        g->n_dev_nodes = N;
        g->pend_nodes.clear();
    }
    if (E > g->n_dev_edges) {
        if (E > g->edge_cap) {
            uint32_t c = g->edge_cap ? g->edge_cap : 1024;
            while (c < E) c *= 2;
            int rc = grow_copy(&g->d_edges, g->n_dev_edges, c, g->st);
            if (rc != LIO_OK) return rc;
            if (g->d_lin) { hipFree(g->d_lin); g->d_lin = nullptr; }
            g->edge_cap = 0;
            LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&g->d_lin), kLinPerEdge * c * sizeof(double)));
            g->edge_cap = c;
            set_lin(g);
        }
        LIO_HIP_TRY(hipMemcpy(g->d_edges + g->n_dev_edges, g->pend_edges.data(), g->pend_edges.size() * sizeof(EdgeDev), hipMemcpyHostToDevice));
        g->n_dev_edges = E;
        g->pend_edges.clear();
    }
    const uint32_t NP = (uint32_t)g->priors.size();
    if (NP > g->n_dev_priors) {
        if (NP > g->prior_cap) {
            uint32_t c = g->prior_cap ? g->prior_cap : 256;
            while (c < NP) c *= 2;
            int rc = grow_copy(&g->d_priors, g->n_dev_priors, c, g->st);
            if (rc != LIO_OK) return rc;
            g->prior_cap = c;
        }
        LIO_HIP_TRY(hipMemcpy(g->d_priors + g->n_dev_priors, g->priors.data() + g->n_dev_priors, (NP - g->n_dev_priors) * sizeof(PriorDev), hipMemcpyHostToDevice));
        g->n_dev_priors = NP;
    }
    const uint32_t nb = (E + kEdgeThreads - 1) / kEdgeThreads;
    if (nb > g->partial_cap) {
        uint32_t c = g->partial_cap ? g->partial_cap : 64;
        while (c < nb) c *= 2;
        if (g->d_partial) hipFree(g->d_partial);
        if (g->h_partial) hipHostFree(g->h_partial);
        g->d_partial = g->h_partial = nullptr;
        g->partial_cap = 0;
        LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&g->d_partial), c * sizeof(double)));
        LIO_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&g->h_partial), c * sizeof(double), hipHostMallocDefault));
        g->partial_cap = c;
    }
    return LIO_OK;
}

// the three CSRs of the live topology
int build_topology(lio_graph* g) {
    if (!g->topo_dirty) return LIO_OK;
    const uint32_t N = num_nodes(g), E = num_edges(g);
    std::vector<uint32_t> deg(N, 0);
    g->n_live = 0;
    for (uint32_t e = 0; e < E; e++)
        if (g->live[e]) { deg[g->from[e]]++; if (g->to[e] >= 0) deg[g->to[e]]++; g->n_live++; }
    std::vector<int32_t> aidx(N, -1);
    g->act.clear();
    for (uint32_t n = 0; n < N; n++)
        if (!g->gone[n] && !g->fixed[n] && deg[n]) { aidx[n] = (int32_t)g->act.size(); g->act.push_back(n); }
    const uint32_t Na = (uint32_t)g->act.size();
    std::vector<std::vector<uint32_t>> dl(Na);
    std::map<std::pair<uint32_t, uint32_t>, std::vector<uint32_t>> pairs;  // (lo, hi) in active indices
    for (uint32_t e = 0; e < E; e++) {
        if (!g->live[e]) continue;
        const int32_t ai = aidx[g->from[e]], aj = g->to[e] >= 0 ? aidx[g->to[e]] : -1;  // a prior: its block sits in the id's Hii / bi slots
        if (ai >= 0) dl[ai].push_back(e << 1);
        if (aj >= 0) dl[aj].push_back(e << 1 | 1u);
        if (ai >= 0 && aj >= 0) {
            if (ai < aj) pairs[{(uint32_t)ai, (uint32_t)aj}].push_back(e << 1);
            else pairs[{(uint32_t)aj, (uint32_t)ai}].push_back(e << 1 | 1u);  // the block (lo, hi) is Hij^T
        }
    }
    const uint32_t P = (uint32_t)pairs.size();
    std::vector<uint32_t> dptr(Na + 1, 0), dlist, pptr(P + 1, 0), plist, rptr(Na + 1, 0), rcol(2ull * P), rblk(2ull * P);
    for (uint32_t a = 0; a < Na; a++) { dlist.insert(dlist.end(), dl[a].begin(), dl[a].end()); dptr[a + 1] = (uint32_t)dlist.size(); }
    std::vector<uint32_t> rcount(Na, 0);
    uint32_t p = 0;
    for (const auto& kv : pairs) {
        plist.insert(plist.end(), kv.second.begin(), kv.second.end());
        pptr[++p] = (uint32_t)plist.size();
        rcount[kv.first.first]++; rcount[kv.first.second]++;
    }
    for (uint32_t a = 0; a < Na; a++) rptr[a + 1] = rptr[a] + rcount[a];
    std::vector<uint32_t> fill(rptr.begin(), rptr.end() - 1);
    p = 0;
    for (const auto& kv : pairs) {  // (lo, hi) ascending: every row's columns come out ascending within {smaller} and {larger}; the order is fixed
        const uint32_t lo = kv.first.first, hi = kv.first.second;
        rcol[fill[lo]] = hi; rblk[fill[lo]++] = p;
        rcol[fill[hi]] = lo; rblk[fill[hi]++] = p | 0x80000000u;
        p++;
    }
    // one allocation of 32-bit words
    const uint64_t words = (uint64_t)Na + (Na + 1) + dlist.size() + (P + 1) + plist.size() + (Na + 1) + 4ull * P + 16;
    if (words > g->topo_cap) {
        uint64_t c = g->topo_cap ? g->topo_cap : 4096;
        while (c < words) c *= 2;
        if (g->d_topo) hipFree(g->d_topo);
        g->d_topo = nullptr; g->topo_cap = 0;
        LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&g->d_topo), c * sizeof(uint32_t)));
        g->topo_cap = c;
    }
    std::vector<uint32_t> host;
    host.reserve(words);
    auto put = [&](const std::vector<uint32_t>& v, uint32_t** d) { *d = g->d_topo + host.size(); host.insert(host.end(), v.begin(), v.end()); };
    put(g->act, &g->d_act); put(dptr, &g->d_dptr); put(dlist, &g->d_dlist); put(pptr, &g->d_pptr); put(plist, &g->d_plist);
    put(rptr, &g->d_rptr); put(rcol, &g->d_rcol); put(rblk, &g->d_rblk);
    if (!host.empty()) LIO_HIP_TRY(hipMemcpy(g->d_topo, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    const uint64_t dbl = 36ull * Na + 36ull * P + 6ull * Na + 36ull * Na + 30ull * Na + 7ull * Na + 16;
    if (dbl > g->sys_cap) {
        uint64_t c = g->sys_cap ? g->sys_cap : 4096;
        while (c < dbl) c *= 2;
        if (g->d_sys) hipFree(g->d_sys);
        g->d_sys = nullptr; g->sys_cap = 0;
        LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&g->d_sys), c * sizeof(double)));
        g->sys_cap = c;
    }
    double* q = g->d_sys;
    g->d_Hd = q; q += 36ull * Na;
    g->d_Ho = q; q += 36ull * P;
    g->d_b = q; q += 6ull * Na;
    g->d_Minv = q; q += 36ull * Na;
    g->d_vec = q; q += 30ull * Na;
    g->d_bak = q;
    g->Na = Na; g->P = P; g->nnz = 2 * P;
    g->topo_dirty = false;
    g->border_stale = true;
    return LIO_OK;
}

// the border's lists and buffers over the current topology: per active node its live XYZ priors, and all of them, by prior index (= rising id)
int build_border(lio_graph* g) {
    const uint32_t Na = g->Na, NP = (uint32_t)g->priors.size();
    std::vector<int32_t> aidx(num_nodes(g), -1);
    for (uint32_t a = 0; a < Na; a++) aidx[g->act[a]] = (int32_t)a;
    std::vector<std::vector<uint32_t>> ml(Na);
    std::vector<uint32_t> all;
    for (uint32_t k = 0; k < NP; k++) {
        const PriorDev& p = g->priors[k];
        if (!p.live || p.type != LIO_GRAPH_PRIOR_XYZ) continue;
        all.push_back(k);
        if (aidx[p.node] >= 0) ml[aidx[p.node]].push_back(k);
    }
    std::vector<uint32_t> host(Na + 1, 0);
    for (uint32_t a = 0; a < Na; a++) host[a + 1] = host[a] + (uint32_t)ml[a].size();
    for (uint32_t a = 0; a < Na; a++) host.insert(host.end(), ml[a].begin(), ml[a].end());
    const uint64_t off_all = host.size();
    host.insert(host.end(), all.begin(), all.end());
    if (host.size() > g->btopo_cap) {
        uint64_t c = g->btopo_cap ? g->btopo_cap : 1024;
        while (c < host.size()) c *= 2;
        if (g->d_btopo) hipFree(g->d_btopo);
        g->d_btopo = nullptr; g->btopo_cap = 0;
        LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&g->d_btopo), c * sizeof(uint32_t)));
        g->btopo_cap = c;
    }
    LIO_HIP_TRY(hipMemcpy(g->d_btopo, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    g->d_mptr = g->d_btopo; g->d_mlist = g->d_btopo + (Na + 1); g->d_mall = g->d_btopo + off_all;
    g->n_mall = (uint32_t)all.size();
    const uint64_t nvec = 6ull * Na + 3, dbl = 9 + 3 + 9 + 18ull * Na + 5 * nvec + (uint64_t)kMlinDoubles * NP + 16;
    if (dbl > g->border_cap) {
        uint64_t c = g->border_cap ? g->border_cap : 4096;
        while (c < dbl) c *= 2;
        if (g->d_border) hipFree(g->d_border);
        g->d_border = nullptr; g->border_cap = 0;
        LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&g->d_border), c * sizeof(double)));
        g->border_cap = c;
    }
    double* q = g->d_border;
    g->d_Hmm = q; q += 9;
    g->d_bm = q; q += 3;
    g->d_Minv3 = q; q += 9;
    g->d_Hpm = q; q += 18ull * Na;
    g->d_bvec = q; q += 5 * nvec;
    g->d_mlin = q;
    g->border_stale = false;
    return LIO_OK;
}

int prepare(lio_graph* g) {
    hipSetDevice(g->device);
    int rc = flush(g);
    if (rc != LIO_OK) return rc;
    rc = build_topology(g);
    if (rc == LIO_OK && g->moment_open && g->border_stale) rc = build_border(g);
    return rc;
}

// between lio_graph_moment_begin and _end the graph's topology is closed
bool moment_refuses(const lio_graph* g, const char* who) {
    if (!g->moment_open) return false;
    set_error("%s: refused between lio_graph_moment_begin and lio_graph_moment_end", who);
    return true;
}

uint32_t grid_for(uint64_t items, uint32_t threads) {
    const uint64_t b = (items + threads - 1) / threads;
    return (uint32_t)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

int launch_linearize(lio_graph* g, int tag) {
    const uint32_t E = num_edges(g);
    if (!E) return LIO_OK;
    hipLaunchKernelGGL(graph_linearize, grid_for(E, kEdgeThreads), kEdgeThreads, 0, g->st, g->d_edges, E, g->d_t, g->d_q, g->d_state, tag, g->lin);
    LIO_HIP_TRY(hipGetLastError());
    const uint32_t NP = (uint32_t)g->priors.size();
    if (NP) {  // after graph_linearize on the same stream: it overwrites the zeros that kernel left at the priors' ids
        hipLaunchKernelGGL(graph_linearize_prior, grid_for(NP, kEdgeThreads), kEdgeThreads, 0, g->st, g->d_priors, NP, g->d_t, g->d_q, g->d_state, tag, g->lin);
        LIO_HIP_TRY(hipGetLastError());
    }
    if (NP && g->moment_open) {  // after graph_linearize_prior: a live XYZ prior's slots are taken again as a moment edge's
        hipLaunchKernelGGL(graph_linearize_moment, grid_for(NP, kEdgeThreads), kEdgeThreads, 0, g->st, g->d_priors, NP, g->d_t, g->d_q, g->d_state, tag, g->lin, g->d_mom,
                           g->d_mlin);
        LIO_HIP_TRY(hipGetLastError());
    }
    return LIO_OK;
}
void launch_chi2(lio_graph* g, int tag, uint32_t nb, uint32_t E) {
    if (g->moment_open)
        hipLaunchKernelGGL(graph_chi2_moment, nb, kEdgeThreads, 0, g->st, g->d_state, tag, g->d_edges, E, g->d_priors, g->d_t, g->d_q, g->d_partial, g->d_mom);
    else if (g->priors.empty())
        hipLaunchKernelGGL(graph_chi2<false>, nb, kEdgeThreads, 0, g->st, g->d_state, tag, g->d_edges, E, g->d_priors, g->d_t, g->d_q, g->d_partial);
    else
        hipLaunchKernelGGL(graph_chi2<true>, nb, kEdgeThreads, 0, g->st, g->d_state, tag, g->d_edges, E, g->d_priors, g->d_t, g->d_q, g->d_partial);
}
int launch_assemble(lio_graph* g, int tag) {
    if (g->moment_open) {
        hipLaunchKernelGGL(graph_assemble_border, grid_for(18ull * g->Na + 12, 256), 256, 0, g->st, g->d_state, tag, g->Na, g->d_mptr, g->d_mlist, g->d_mall, g->n_mall,
                           g->d_mlin, g->d_mom, g->d_Hpm, g->d_Hmm, g->d_bm);
        LIO_HIP_TRY(hipGetLastError());
    }
    if (!g->Na) return LIO_OK;
    const uint64_t items = 36ull * g->Na + 36ull * g->P + 6ull * g->Na;
    hipLaunchKernelGGL(graph_assemble, grid_for(items, 256), 256, 0, g->st, g->d_state, tag, g->Na, g->P, g->d_dptr, g->d_dlist, g->d_pptr, g->d_plist, g->lin, g->d_Hd,
                       g->d_Ho, g->d_b);
    LIO_HIP_TRY(hipGetLastError());
    return LIO_OK;
}
// the graph's chi2 at the current estimate: the partials folded in order (graph_decide's fold)
int chi2_now(lio_graph* g, double* out) {
    const uint32_t E = num_edges(g);
    double c = 0.0;
    if (E) {
        const uint32_t nb = (E + kEdgeThreads - 1) / kEdgeThreads;
        launch_chi2(g, -1, nb, E);
        LIO_HIP_TRY(hipGetLastError());
        LIO_HIP_TRY(hipMemcpyAsync(g->h_partial, g->d_partial, nb * sizeof(double), hipMemcpyDeviceToHost, g->st));
        LIO_HIP_TRY(hipStreamSynchronize(g->st));
        for (uint32_t k = 0; k < nb; k++) c += g->h_partial[k];
    }
    if (g->moment_open) {  // the moment's own prior, after the partials as graph_decide adds it
        double m[3];
        LIO_HIP_TRY(hipMemcpyAsync(m, g->d_mom + kMomM, sizeof(m), hipMemcpyDeviceToHost, g->st));
        LIO_HIP_TRY(hipStreamSynchronize(g->st));
        c += moment_prior_chi2(m, g->moment_info);
    }
    *out = c;
    return LIO_OK;
}

bool pose_ok(const double T[16]) {
    for (int k = 0; k < 16; k++)
        if (!(T[k] - T[k] == 0.0)) return false;
    return true;
}

bool kernel_ok(const char* who, int kernel, double delta) {
    if (kernel != LIO_GRAPH_KERNEL_NONE && kernel != LIO_GRAPH_KERNEL_HUBER && kernel != LIO_GRAPH_KERNEL_DCS2) { set_error("%s: unknown kernel %d", who, kernel); return false; }
    if (kernel != LIO_GRAPH_KERNEL_NONE && !(delta > 0)) { set_error("%s: a robust kernel needs a positive delta", who); return false; }
    return true;
}

// kernel, delta and live of one prior: the host mirror, and the device's record when it is there already
int prior_set(lio_graph* g, uint32_t slot, int kernel, double delta, int live) {
    PriorDev& p = g->priors[slot];
    p.kernel = kernel; p.delta = delta; p.live = live;
    if (slot < g->n_dev_priors) LIO_HIP_TRY(hipMemcpy(g->d_priors + slot, &p, sizeof(PriorDev), hipMemcpyHostToDevice));
    return LIO_OK;
}

void free_all(lio_graph* g) {
    hipFree(g->d_t); hipFree(g->d_q); hipFree(g->d_edges); hipFree(g->d_priors); hipFree(g->d_lin); hipFree(g->d_topo); hipFree(g->d_sys); hipFree(g->d_partial); hipFree(g->d_state);
    hipFree(g->d_mom); hipFree(g->d_border); hipFree(g->d_btopo);
    if (g->h_partial) hipHostFree(g->h_partial);
    if (g->h_state) hipHostFree(g->h_state);
}

}  // namespace

extern "C" {

void lio_graph_default_params(lio_graph_params* p) {
    if (!p) return;
    p->cg_epsilon = 1e-10;
    p->chi2_rel_stop = 0.0;
    p->min_edges = 10;
    p->cg_max_iterations = 0;
}

void lio_se3_from_mqt(const double v6[6], double T16[16]) {
    if (!v6 || !T16) return;
    double t[3] = {0, 0, 0}, q[4] = {0, 0, 0, 1};
    apply_delta(t, q, v6);  // from the identity: t = v[0:3], q = (v[3:6], w) or the identity rotation
    tq_to_T(t, q, T16);
}
void lio_se3_to_mqt(const double T16[16], double v6[6]) {
    if (!v6 || !T16) return;
    double t[3], q[4];
    T_to_tq(T16, t, q);
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; }
    v6[0] = t[0]; v6[1] = t[1]; v6[2] = t[2]; v6[3] = q[0]; v6[4] = q[1]; v6[5] = q[2];
}
int lio_graph_edge_error(const double Xfrom16[16], const double Xto16[16], const double M16[16], double e6[6]) {
    if (!Xfrom16 || !Xto16 || !M16 || !e6) return LIO_E_INVALID;
    double ti[3], qi[4], tj[3], qj[4], mt[3], mq[4], tb[3], qb[4], qe[4];
    T_to_tq(Xfrom16, ti, qi); T_to_tq(Xto16, tj, qj); T_to_tq(M16, mt, mq);
    edge_eval(ti, qi, tj, qj, mt, mq, e6, tb, qb, qe);
    return LIO_OK;
}

lio_graph* lio_graph_create(int device, const lio_graph_params* params) {
    lio_graph_params p;
    if (params) p = *params; else lio_graph_default_params(&p);
    if (!(p.cg_epsilon > 0) || !(p.chi2_rel_stop >= 0) || p.min_edges < 0 || p.cg_max_iterations < 0) {
        set_error("lio_graph_create: cg_epsilon must be positive, chi2_rel_stop, min_edges and cg_max_iterations not negative");
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) { set_error("lio_graph_create: no HIP device %d (this library has no CPU fallback)", device); return nullptr; }
    lio_graph* g = new lio_graph();
    g->device = device;
    g->par = p;
    bool ok = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&g->d_state), sizeof(LmState)) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void**>(&g->h_state), sizeof(LmState), hipHostMallocDefault) == hipSuccess;
    for (int i = 0; ok && i < kEvents; i++) ok = hipEventCreate(&g->ev[i]) == hipSuccess;
    if (ok) { memset(g->h_state, 0, sizeof(LmState)); ok = hipMemset(g->d_state, 0, sizeof(LmState)) == hipSuccess; }
    if (!ok) { set_error("lio_graph_create: allocation failed"); lio_graph_destroy(g); return nullptr; }
    return g;
}

void lio_graph_destroy(lio_graph* g) {
    if (!g) return;
    hipSetDevice(g->device);
    if (g->st) hipStreamSynchronize(g->st);
    free_all(g);
    for (int i = 0; i < kEvents; i++)
        if (g->ev[i]) hipEventDestroy(g->ev[i]);
    if (g->st) hipStreamDestroy(g->st);
    delete g;
}

int lio_graph_reset(lio_graph* g) {
    if (!g) return LIO_E_INVALID;
    if (moment_refuses(g, "lio_graph_reset")) return LIO_E_STATE;
    hipSetDevice(g->device);
    LIO_HIP_TRY(hipStreamSynchronize(g->st));
    g->from.clear(); g->to.clear(); g->pslot.clear(); g->live.clear(); g->fixed.clear(); g->gone.clear(); g->rec.clear(); g->pend_nodes.clear(); g->pend_edges.clear(); g->priors.clear();
    g->n_dev_nodes = g->n_dev_edges = g->n_dev_priors = 0;
    g->topo_dirty = true;
    g->Na = g->P = g->n_live = 0;
    memset(&g->rep, 0, sizeof(g->rep));
    g->t_lin = g->t_asm = g->t_solve = g->t_update = 0;
    return LIO_OK;
}

int lio_graph_add_node(lio_graph* g, const double pose16[16]) {
    if (!g || !pose16 || !pose_ok(pose16)) return LIO_E_INVALID;
    if (moment_refuses(g, "lio_graph_add_node")) return LIO_E_STATE;
    double t[3], q[4];
    T_to_tq(pose16, t, q);
    g->pend_nodes.insert(g->pend_nodes.end(), t, t + 3);
    g->pend_nodes.insert(g->pend_nodes.end(), q, q + 4);
    g->fixed.push_back(0);
    g->gone.push_back(0);
    g->topo_dirty = true;
    return (int)g->fixed.size() - 1;
}

int lio_graph_set_fixed(lio_graph* g, int id, int flag) {
    if (!g || !node_ok(g, id)) return LIO_E_INVALID;
    const uint8_t f = flag ? 1 : 0;
    if (g->fixed[id] != f) { g->fixed[id] = f; g->topo_dirty = true; }
    return LIO_OK;
}

int lio_graph_set_estimate(lio_graph* g, int id, const double pose16[16]) {
    if (!g || !node_ok(g, id) || !pose16 || !pose_ok(pose16)) return LIO_E_INVALID;
    double tq[7];
    T_to_tq(pose16, tq, tq + 3);
    if ((uint32_t)id >= g->n_dev_nodes) {
        memcpy(&g->pend_nodes[7ull * ((uint32_t)id - g->n_dev_nodes)], tq, sizeof(tq));
        return LIO_OK;
    }
    hipSetDevice(g->device);
    LIO_HIP_TRY(hipMemcpy(g->d_t + 3ull * id, tq, 3 * sizeof(double), hipMemcpyHostToDevice));
    LIO_HIP_TRY(hipMemcpy(g->d_q + 4ull * id, tq + 3, 4 * sizeof(double), hipMemcpyHostToDevice));
    return LIO_OK;
}

int lio_graph_add_edge(lio_graph* g, int from, int to, const double M16[16], const double info36[36], int kernel, double delta) {
    if (!g || !M16 || !info36 || !node_ok(g, from) || !node_ok(g, to) || !pose_ok(M16)) return LIO_E_INVALID;
    if (moment_refuses(g, "lio_graph_add_edge")) return LIO_E_STATE;
    if (from == to) { set_error("lio_graph_add_edge: an edge from node %d to itself", from); return LIO_E_INVALID; }
    if (!kernel_ok("lio_graph_add_edge", kernel, delta)) return LIO_E_INVALID;
    double amax = 0.0;
    for (int k = 0; k < 36; k++) {
        if (!(info36[k] - info36[k] == 0.0)) { set_error("lio_graph_add_edge: the information matrix is not finite"); return LIO_E_INVALID; }
        amax = fmax(amax, fabs(info36[k]));
    }
    for (int r = 0; r < 6; r++)
        for (int c = r + 1; c < 6; c++)
            if (fabs(info36[r * 6 + c] - info36[c * 6 + r]) > 1e-9 * amax) { set_error("lio_graph_add_edge: the information matrix is not symmetric"); return LIO_E_INVALID; }
    EdgeDev e{};
    e.from = from; e.to = to; e.kernel = kernel; e.live = 1; e.delta = delta;
    T_to_tq(M16, e.mt, e.mq);
    memcpy(e.info, info36, sizeof(e.info));
    g->pend_edges.push_back(e);
    lio_graph::EdgeRec r;
    memcpy(r.M, M16, sizeof(r.M)); memcpy(r.info, info36, sizeof(r.info));
    r.kernel = kernel; r.delta = delta;
    g->rec.push_back(r);
    g->from.push_back(from); g->to.push_back(to); g->pslot.push_back(-1); g->live.push_back(1);
    g->topo_dirty = true;
    return (int)g->from.size() - 1;
}

int lio_graph_add_prior(lio_graph* g, int node, int type, const double m4[4], const double plane4[4], const double info9[9], int kernel, double delta) {
    if (!g || !m4 || !info9 || !node_ok(g, node)) return LIO_E_INVALID;
    if (moment_refuses(g, "lio_graph_add_prior")) return LIO_E_STATE;
    if (type != LIO_GRAPH_PRIOR_XYZ && type != LIO_GRAPH_PRIOR_QUAT && type != LIO_GRAPH_PRIOR_PLANE) { set_error("lio_graph_add_prior: unknown type %d", type); return LIO_E_INVALID; }
    if (type == LIO_GRAPH_PRIOR_PLANE && !plane4) { set_error("lio_graph_add_prior: a PLANE prior needs its world plane"); return LIO_E_INVALID; }
    if (!kernel_ok("lio_graph_add_prior", kernel, delta) || !(delta - delta == 0.0)) return LIO_E_INVALID;
    PriorDev p{};
    p.node = node; p.type = type; p.kernel = kernel; p.live = 1; p.delta = delta;
    const int nm = type == LIO_GRAPH_PRIOR_XYZ ? 3 : 4;
    for (int k = 0; k < nm; k++) {
        if (!(m4[k] - m4[k] == 0.0)) { set_error("lio_graph_add_prior: the measurement is not finite"); return LIO_E_INVALID; }
        p.m[k] = m4[k];
    }
    if (type == LIO_GRAPH_PRIOR_QUAT) {  // normalised, w >= 0
        const double n = sqrt(((p.m[0] * p.m[0] + p.m[1] * p.m[1]) + p.m[2] * p.m[2]) + p.m[3] * p.m[3]);
        if (!(n > 0) || !(n - n == 0.0)) { set_error("lio_graph_add_prior: a zero quaternion"); return LIO_E_INVALID; }
        const double s = p.m[3] < 0 ? -1.0 : 1.0;
        for (int k = 0; k < 4; k++) p.m[k] = s * (p.m[k] / n);
    } else if (type == LIO_GRAPH_PRIOR_PLANE) {  // both planes divided by the norm of their normal
        for (int k = 0; k < 4; k++) {
            if (!(plane4[k] - plane4[k] == 0.0)) { set_error("lio_graph_add_prior: the world plane is not finite"); return LIO_E_INVALID; }
            p.plane[k] = plane4[k];
        }
        for (double* v : {p.m, p.plane}) {
            const double n = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
            if (!(n > 0) || !(n - n == 0.0)) { set_error("lio_graph_add_prior: a plane with a zero normal"); return LIO_E_INVALID; }
            for (int k = 0; k < 4; k++) v[k] /= n;
        }
    }
    double amax = 0.0;
    for (int k = 0; k < 9; k++) {
        if (!(info9[k] - info9[k] == 0.0)) { set_error("lio_graph_add_prior: the information matrix is not finite"); return LIO_E_INVALID; }
        amax = fmax(amax, fabs(info9[k]));
    }
    for (int r = 0; r < 3; r++)
        for (int c = r + 1; c < 3; c++)
            if (fabs(info9[r * 3 + c] - info9[c * 3 + r]) > 1e-9 * amax) { set_error("lio_graph_add_prior: the information matrix is not symmetric"); return LIO_E_INVALID; }
    memcpy(p.info, info9, sizeof(p.info));
    p.id = (int32_t)g->from.size();
    EdgeDev hole{};  // the id's place in the edge array
    hole.from = (int32_t)g->priors.size(); hole.to = -1; hole.live = kPriorSlot;
    g->pend_edges.push_back(hole);
    g->priors.push_back(p);
    g->rec.push_back(lio_graph::EdgeRec());
    g->from.push_back(node); g->to.push_back(-1); g->pslot.push_back(hole.from); g->live.push_back(1);
    g->topo_dirty = true;
    return p.id;
}

int lio_graph_set_kernel(lio_graph* g, int id, int kernel, double delta) {
    if (!g || id < 0 || (uint32_t)id >= num_edges(g) || !g->live[id]) return LIO_E_INVALID;
    if (!kernel_ok("lio_graph_set_kernel", kernel, delta) || !(delta - delta == 0.0)) return LIO_E_INVALID;
    hipSetDevice(g->device);
    if (g->pslot[id] >= 0) return prior_set(g, (uint32_t)g->pslot[id], kernel, delta, 1);
    g->rec[id].kernel = kernel; g->rec[id].delta = delta;
    if ((uint32_t)id >= g->n_dev_edges) {
        EdgeDev& e = g->pend_edges[(uint32_t)id - g->n_dev_edges];
        e.kernel = kernel; e.delta = delta;
        return LIO_OK;
    }
    const int32_t k = kernel;
    LIO_HIP_TRY(hipMemcpy(&g->d_edges[id].kernel, &k, sizeof(k), hipMemcpyHostToDevice));
    LIO_HIP_TRY(hipMemcpy(&g->d_edges[id].delta, &delta, sizeof(delta), hipMemcpyHostToDevice));
    return LIO_OK;
}

int lio_graph_priors(lio_graph* g, int32_t* id, int32_t* node, int32_t* type, double* m4, double* plane4, double* info9, int32_t* kernel, double* delta, uint32_t cap) {
    if (!g) return LIO_E_INVALID;
    uint32_t n = 0;
    for (const PriorDev& p : g->priors) n += p.live ? 1 : 0;
    if (n > cap) return -(int)n;
    uint32_t k = 0;
    for (const PriorDev& p : g->priors) {
        if (!p.live) continue;
        if (id) id[k] = p.id;
        if (node) node[k] = p.node;
        if (type) type[k] = p.type;
        if (m4) memcpy(m4 + 4ull * k, p.m, sizeof(p.m));
        if (plane4) memcpy(plane4 + 4ull * k, p.plane, sizeof(p.plane));
        if (info9) memcpy(info9 + 9ull * k, p.info, sizeof(p.info));
        if (kernel) kernel[k] = p.kernel;
        if (delta) delta[k] = p.delta;
        k++;
    }
    return (int)n;
}

int lio_graph_prior_error(const double X16[16], int type, const double m4[4], const double plane4[4], double e3[3]) {
    if (!X16 || !m4 || !e3 || (type != LIO_GRAPH_PRIOR_XYZ && type != LIO_GRAPH_PRIOR_QUAT && type != LIO_GRAPH_PRIOR_PLANE) || (type == LIO_GRAPH_PRIOR_PLANE && !plane4))
        return LIO_E_INVALID;
    double t[3], q[4], m[4] = {m4[0], m4[1], m4[2], type == LIO_GRAPH_PRIOR_XYZ ? 0.0 : m4[3]}, pl[4] = {0, 0, 0, 0}, A[9], nl[3], u[3], sgn = 1.0;
    T_to_tq(X16, t, q);
    if (type == LIO_GRAPH_PRIOR_QUAT) {
        const double n = sqrt(((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) + m[3] * m[3]);
        if (!(n > 0)) return LIO_E_INVALID;
        const double s = m[3] < 0 ? -1.0 : 1.0;
        for (int k = 0; k < 4; k++) m[k] = s * (m[k] / n);
    } else if (type == LIO_GRAPH_PRIOR_PLANE) {
        memcpy(pl, plane4, sizeof(pl));
        for (double* v : {m, pl}) {
            const double n = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
            if (!(n > 0)) return LIO_E_INVALID;
            for (int k = 0; k < 4; k++) v[k] /= n;
        }
    }
    prior_eval(type, t, q, m, pl, e3, A, nl, u, &sgn);
    return LIO_OK;
}

int lio_graph_remove_edge(lio_graph* g, int id) {
    if (!g || id < 0 || (uint32_t)id >= num_edges(g) || !g->live[id]) return LIO_E_INVALID;
    if (moment_refuses(g, "lio_graph_remove_edge")) return LIO_E_STATE;
    g->live[id] = 0;
    g->topo_dirty = true;
    if (g->pslot[id] >= 0) {  // the placeholder stays; the prior's own record goes dead
        hipSetDevice(g->device);
        const PriorDev& p = g->priors[g->pslot[id]];
        return prior_set(g, (uint32_t)g->pslot[id], p.kernel, p.delta, 0);
    }
    if ((uint32_t)id >= g->n_dev_edges) { g->pend_edges[(uint32_t)id - g->n_dev_edges].live = 0; return LIO_OK; }
    hipSetDevice(g->device);
    const int32_t zero = 0;
    LIO_HIP_TRY(hipMemcpy(&g->d_edges[id].live, &zero, sizeof(zero), hipMemcpyHostToDevice));
    return LIO_OK;
}

int lio_graph_remove_node(lio_graph* g, int id) {
    if (!g || !node_ok(g, id)) return LIO_E_INVALID;
    if (moment_refuses(g, "lio_graph_remove_node")) return LIO_E_STATE;
    for (uint32_t e = 0; e < num_edges(g); e++) {  // g2o's removeVertex: every edge and prior on the node goes with it
        if (!g->live[e] || (g->from[e] != id && g->to[e] != id)) continue;
        const int rc = lio_graph_remove_edge(g, (int)e);
        if (rc != LIO_OK) return rc;
    }
    g->gone[id] = 1;
    g->fixed[id] = 0;
    g->topo_dirty = true;
    return LIO_OK;
}

int lio_graph_node_live(lio_graph* g, uint8_t* out, uint32_t cap) {
    if (!g) return LIO_E_INVALID;
    const uint32_t N = num_nodes(g);
    if (N > cap || (N && !out)) return -(int)N;
    for (uint32_t n = 0; n < N; n++) out[n] = g->gone[n] ? 0 : 1;
    return (int)N;
}

int lio_graph_edge_records(lio_graph* g, int32_t* id, int32_t* from, int32_t* to, double* M16, double* info36, int32_t* kernel, double* delta, uint32_t cap) {
    if (!g) return LIO_E_INVALID;
    uint32_t n = 0;
    for (uint32_t e = 0; e < num_edges(g); e++) n += (g->live[e] && g->pslot[e] < 0) ? 1 : 0;
    if (n > cap) return -(int)n;
    uint32_t k = 0;
    for (uint32_t e = 0; e < num_edges(g); e++) {
        if (!g->live[e] || g->pslot[e] >= 0) continue;
        const lio_graph::EdgeRec& r = g->rec[e];
        if (id) id[k] = (int32_t)e;
        if (from) from[k] = g->from[e];
        if (to) to[k] = g->to[e];
        if (M16) memcpy(M16 + 16ull * k, r.M, sizeof(r.M));
        if (info36) memcpy(info36 + 36ull * k, r.info, sizeof(r.info));
        if (kernel) kernel[k] = r.kernel;
        if (delta) delta[k] = r.delta;
        k++;
    }
    return (int)n;
}

int lio_graph_num_nodes(lio_graph* g) { return g ? (int)num_nodes(g) : LIO_E_INVALID; }

int lio_graph_chi2(lio_graph* g, double* chi2) {
    if (!g || !chi2) return LIO_E_INVALID;
    int rc = prepare(g);
    if (rc != LIO_OK) return rc;
    return chi2_now(g, chi2);
}

int lio_graph_estimates(lio_graph* g, double* out16, uint32_t cap) {
    if (!g) return LIO_E_INVALID;
    const uint32_t N = num_nodes(g);
    if (N > cap || (N && !out16)) return -(int)N;
    if (!N) return 0;
    int rc = prepare(g);
    if (rc != LIO_OK) return rc;
    std::vector<double> t(3ull * N), q(4ull * N);
    LIO_HIP_TRY(hipMemcpy(t.data(), g->d_t, t.size() * sizeof(double), hipMemcpyDeviceToHost));
    LIO_HIP_TRY(hipMemcpy(q.data(), g->d_q, q.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (uint32_t n = 0; n < N; n++) tq_to_T(&t[3ull * n], &q[4ull * n], out16 + 16ull * n);
    return (int)N;
}

int lio_graph_edges(lio_graph* g, int32_t* from, int32_t* to, int32_t* id, uint32_t cap) {
    if (!g) return LIO_E_INVALID;
    uint32_t n = 0;
    for (uint32_t e = 0; e < num_edges(g); e++) n += g->live[e];
    if (n > cap) return -(int)n;
    uint32_t k = 0;
    for (uint32_t e = 0; e < num_edges(g); e++) {
        if (!g->live[e]) continue;
        if (from) from[k] = g->from[e];
        if (to) to[k] = g->to[e];
        if (id) id[k] = (int32_t)e;
        k++;
    }
    return (int)n;
}

int lio_graph_get_fixed(lio_graph* g, uint8_t* out, uint32_t cap) {
    if (!g) return LIO_E_INVALID;
    const uint32_t N = num_nodes(g);
    if (N > cap || (N && !out)) return -(int)N;
    for (uint32_t n = 0; n < N; n++) out[n] = g->fixed[n];
    return (int)N;
}

int lio_graph_linearize(lio_graph* g, double* errors, double* chi2, double* rho1, uint32_t edge_cap, double* b, double* Hdiag, uint32_t node_cap) {
    if (!g) return LIO_E_INVALID;
    const uint32_t N = num_nodes(g), E = num_edges(g);
    if (((errors || chi2 || rho1) && E > edge_cap) || ((b || Hdiag) && N > node_cap)) return LIO_E_CAPACITY;
    int rc = prepare(g);
    if (rc != LIO_OK) return rc;
    rc = launch_linearize(g, -1);
    if (rc == LIO_OK) rc = launch_assemble(g, -1);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipStreamSynchronize(g->st));
    if (E) {
        if (errors) LIO_HIP_TRY(hipMemcpy(errors, g->lin.err, 6ull * E * sizeof(double), hipMemcpyDeviceToHost));
        if (chi2) LIO_HIP_TRY(hipMemcpy(chi2, g->lin.chi2, (uint64_t)E * sizeof(double), hipMemcpyDeviceToHost));
        if (rho1) LIO_HIP_TRY(hipMemcpy(rho1, g->lin.rho1, (uint64_t)E * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (b) memset(b, 0, 6ull * N * sizeof(double));
    if (Hdiag) memset(Hdiag, 0, 36ull * N * sizeof(double));
    if (g->Na && (b || Hdiag)) {
        std::vector<double> hb(6ull * g->Na), hd(36ull * g->Na);
        LIO_HIP_TRY(hipMemcpy(hb.data(), g->d_b, hb.size() * sizeof(double), hipMemcpyDeviceToHost));
        LIO_HIP_TRY(hipMemcpy(hd.data(), g->d_Hd, hd.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (uint32_t a = 0; a < g->Na; a++) {
            if (b) memcpy(b + 6ull * g->act[a], &hb[6ull * a], 6 * sizeof(double));
            if (Hdiag) memcpy(Hdiag + 36ull * g->act[a], &hd[36ull * a], 36 * sizeof(double));
        }
    }
    return (int)E;
}

int lio_graph_optimize(lio_graph* g, int max_iterations, lio_graph_report* report) {
    if (!g) return LIO_E_INVALID;
    uint32_t n_live = 0;
    for (uint32_t e = 0; e < num_edges(g); e++) n_live += g->live[e];
    const bool border = g->moment_open;
    if (border) n_live++;  // the moment's own prior is a live edge
    if ((int64_t)n_live < (int64_t)g->par.min_edges) return -1;  // GraphSLAM::optimize: nothing is touched
    int rc = prepare(g);
    if (rc != LIO_OK) return rc;
    lio_graph_report& R = g->rep;
    memset(&R, 0, sizeof(R));
    g->t_lin = g->t_asm = g->t_solve = g->t_update = 0;
    R.n_active = (int32_t)g->Na;
    R.n_live_edges = (int32_t)n_live;
    double c0 = 0.0;
    rc = chi2_now(g, &c0);
    if (rc != LIO_OK) return rc;
    R.chi2_initial = R.chi2_final = c0;
    if (max_iterations <= 0 || (g->Na == 0 && !border) || num_edges(g) == 0) { if (report) *report = R; return 0; }
    LmState& S = *g->h_state;
    memset(&S, 0, sizeof(S));
    S.chi2 = c0; S.nu = 2.0; S.need_lambda_init = 1;
    LIO_HIP_TRY(hipMemcpyAsync(g->d_state, g->h_state, sizeof(LmState), hipMemcpyHostToDevice, g->st));
    const uint32_t E = num_edges(g), nb = (E + kEdgeThreads - 1) / kEdgeThreads, Na = g->Na;
    const int cg_max = g->par.cg_max_iterations > 0 ? g->par.cg_max_iterations : (Na ? (int)(12u * Na) : 3);  // (Na = 0: the border's three unknowns alone)
    const BorderArgs B{g->d_Hpm, g->d_Hmm, g->d_bm, g->d_Minv3};
    for (int it = 0; it < max_iterations; it++) {
        int ne = 0;
        hipEventRecord(g->ev[ne++], g->st);
        rc = launch_linearize(g, it);
        if (rc != LIO_OK) return rc;
        hipEventRecord(g->ev[ne++], g->st);
        rc = launch_assemble(g, it);
        if (rc != LIO_OK) return rc;
        hipEventRecord(g->ev[ne++], g->st);
        for (int trial = 0; border && trial < kMaxTrials; trial++) {  // the same trial over the bordered system
            hipLaunchKernelGGL(graph_solve_border, 1, kSolveThreads, 0, g->st, g->d_state, it, Na, g->d_Hd, g->d_Ho, g->d_b, g->d_rptr, g->d_rcol, g->d_rblk, g->d_Minv,
                               g->d_bvec, g->par.cg_epsilon, cg_max, B);
            hipEventRecord(g->ev[ne++], g->st);
            if (Na) hipLaunchKernelGGL(graph_update, (Na + 255) / 256, 256, 0, g->st, g->d_state, it, Na, g->d_act, g->d_bvec, g->d_t, g->d_q, g->d_bak);
            hipLaunchKernelGGL(graph_update_moment, 1, 64, 0, g->st, g->d_state, it, g->d_bvec + 6ull * Na, g->d_mom);
            launch_chi2(g, it, nb, E);
            hipLaunchKernelGGL(graph_decide_moment, 1, 256, 0, g->st, g->d_state, it, g->d_partial, nb, Na, g->d_act, g->d_bak, g->d_t, g->d_q, max_iterations,
                               g->par.chi2_rel_stop, g->d_mom);
            hipEventRecord(g->ev[ne++], g->st);
        }
        for (int trial = 0; !border && trial < kMaxTrials; trial++) {
            hipLaunchKernelGGL(graph_solve, 1, kSolveThreads, 0, g->st, g->d_state, it, Na, g->d_Hd, g->d_Ho, g->d_b, g->d_rptr, g->d_rcol, g->d_rblk, g->d_Minv, g->d_vec,
                               g->par.cg_epsilon, cg_max);
            hipEventRecord(g->ev[ne++], g->st);
            hipLaunchKernelGGL(graph_update, (Na + 255) / 256, 256, 0, g->st, g->d_state, it, Na, g->d_act, g->d_vec, g->d_t, g->d_q, g->d_bak);
            launch_chi2(g, it, nb, E);
            hipLaunchKernelGGL(graph_decide, 1, 256, 0, g->st, g->d_state, it, g->d_partial, nb, Na, g->d_act, g->d_bak, g->d_t, g->d_q, max_iterations, g->par.chi2_rel_stop);
            hipEventRecord(g->ev[ne++], g->st);
        }
        LIO_HIP_TRY(hipGetLastError());
        LIO_HIP_TRY(hipMemcpyAsync(g->h_state, g->d_state, sizeof(LmState), hipMemcpyDeviceToHost, g->st));
        LIO_HIP_TRY(hipStreamSynchronize(g->st));
        for (int k = 0; k + 1 < ne; k++) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, g->ev[k], g->ev[k + 1]) != hipSuccess) continue;
            double* acc = k == 0 ? &g->t_lin : k == 1 ? &g->t_asm : (k % 2 == 0 ? &g->t_solve : &g->t_update);
            *acc += (double)ms * 1000.0;
        }
        if (S.stop || S.batch != it + 1) break;
    }
    R.iterations = S.iteration;
    R.stop_reason = S.stop;
    R.trials = S.total_trials;
    R.accepted = S.accepted;
    R.cg_iterations = S.cg_iterations;
    R.cg_iterations_total = S.cg_total;
    R.chi2_final = S.chi2;
    R.lambda = S.lambda;
    R.cg_residual = S.cg_relres;
    if (report) *report = R;
    if (S.batch != S.iteration) { set_error("lio_graph_optimize: an iteration did not finish on the device"); return LIO_E_STATE; }
    return S.iteration;
}

int lio_graph_remove_gnss_outliers(lio_graph* g, double max_distance_error, int max_iterations, int32_t* removed_ids, uint32_t cap, lio_graph_report* report) {
    if (!g || !(max_distance_error > 0)) return LIO_E_INVALID;
    if (moment_refuses(g, "lio_graph_remove_gnss_outliers")) return LIO_E_STATE;
    uint32_t n_live = 0;
    for (uint32_t e = 0; e < num_edges(g); e++) n_live += g->live[e];
    if ((int64_t)n_live < (int64_t)g->par.min_edges) return -1;
    hipSetDevice(g->device);
    std::vector<uint32_t> gnss;
    for (uint32_t k = 0; k < g->priors.size(); k++) {
        const PriorDev& p = g->priors[k];
        if (!p.live || p.type != LIO_GRAPH_PRIOR_XYZ) continue;
        const double phi = max_distance_error * max_distance_error * p.info[0];
        if (!(phi > 0)) { set_error("lio_graph_remove_gnss_outliers: prior %d has no positive information(0, 0)", p.id); return LIO_E_INVALID; }
        gnss.push_back(k);
    }
    for (uint32_t k : gnss) {
        const PriorDev& p = g->priors[k];
        int rc = prior_set(g, k, LIO_GRAPH_KERNEL_DCS2, max_distance_error * max_distance_error * p.info[0], 1);
        if (rc != LIO_OK) return rc;
    }
    int rc = lio_graph_optimize(g, max_iterations, report);
    if (rc < 0) return rc == -1 ? LIO_E_STATE : rc;
    int removed = 0;
    if (!gnss.empty()) {
        const uint32_t E = num_edges(g);
        std::vector<double> chi2(E);
        rc = lio_graph_linearize(g, nullptr, chi2.data(), nullptr, E, nullptr, nullptr, 0);
        if (rc < 0) return rc;
        for (uint32_t k : gnss) {
            const PriorDev& p = g->priors[k];
            if (!((2.0 * p.delta) / (p.delta + chi2[p.id]) < 0.1)) continue;
            if (removed_ids && (uint32_t)removed < cap) removed_ids[removed] = p.id;
            rc = lio_graph_remove_edge(g, p.id);
            if (rc != LIO_OK) return rc;
            removed++;
        }
    }
    rc = lio_graph_optimize(g, max_iterations, report);
    if (rc < -1) return rc;
    return removed;
}

int lio_graph_moment_begin(lio_graph* g, const double m0[3], const double info9[9]) {
    if (!g) return LIO_E_INVALID;
    if (moment_refuses(g, "lio_graph_moment_begin")) return LIO_E_STATE;
    double mom[kMomDoubles] = {};
    const double ref[9] = {1.0 / 2000.0, 0, 0, 0, 1.0 / 2000.0, 0, 0, 0, 1.0 / 200.0};  // hdl_graph_slam_nodelet.cpp:1041-1043
    for (int k = 0; k < 3; k++) mom[kMomM + k] = mom[kMomBak + k] = m0 ? m0[k] : 0.0;
    double amax = 0.0;
    for (int k = 0; k < 9; k++) { mom[kMomInfo + k] = info9 ? info9[k] : ref[k]; amax = fmax(amax, fabs(mom[kMomInfo + k])); }
    for (int k = 0; k < kMomDoubles; k++)
        if (!(mom[k] - mom[k] == 0.0)) { set_error("lio_graph_moment_begin: the moment or its information is not finite"); return LIO_E_INVALID; }
    for (int r = 0; r < 3; r++)
        for (int c = r + 1; c < 3; c++)
            if (fabs(mom[kMomInfo + r * 3 + c] - mom[kMomInfo + c * 3 + r]) > 1e-9 * amax) { set_error("lio_graph_moment_begin: the information matrix is not symmetric"); return LIO_E_INVALID; }
    hipSetDevice(g->device);
    if (!g->d_mom) LIO_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&g->d_mom), kMomDoubles * sizeof(double)));
    LIO_HIP_TRY(hipMemcpy(g->d_mom, mom, sizeof(mom), hipMemcpyHostToDevice));
    memcpy(g->moment_info, mom + kMomInfo, sizeof(g->moment_info));
    g->moment_open = true;
    g->border_stale = true;
    const int rc = prepare(g);
    if (rc != LIO_OK) g->moment_open = false;
    return rc;
}

int lio_graph_moment_get(lio_graph* g, double m3[3]) {
    if (!g || !m3) return LIO_E_INVALID;
    if (!g->moment_open) { set_error("lio_graph_moment_get: no moment stage is open"); return LIO_E_STATE; }
    hipSetDevice(g->device);
    LIO_HIP_TRY(hipStreamSynchronize(g->st));
    LIO_HIP_TRY(hipMemcpy(m3, g->d_mom + kMomM, 3 * sizeof(double), hipMemcpyDeviceToHost));
    return LIO_OK;
}

int lio_graph_moment_end(lio_graph* g, int apply) {
    if (!g) return LIO_E_INVALID;
    if (!g->moment_open) { set_error("lio_graph_moment_end: no moment stage is open"); return LIO_E_STATE; }
    int moved = 0;
    if (apply) {  // every moment edge is an XYZ prior again: z' = z + R_node m, in place (its id, information and kernel stay)
        double m[3];
        int rc = lio_graph_moment_get(g, m);
        if (rc != LIO_OK) return rc;
        const uint32_t N = num_nodes(g), NP = (uint32_t)g->priors.size();
        std::vector<double> q(4ull * N);
        if (N) LIO_HIP_TRY(hipMemcpy(q.data(), g->d_q, q.size() * sizeof(double), hipMemcpyDeviceToHost));
        uint32_t first = NP;
        for (uint32_t k = 0; k < NP; k++) {
            PriorDev& p = g->priors[k];
            if (!p.live || p.type != LIO_GRAPH_PRIOR_XYZ) continue;
            double R[9];
            q_to_R(&q[4ull * p.node], R);
            for (int r = 0; r < 3; r++) p.m[r] = p.m[r] + ((R[r * 3] * m[0] + R[r * 3 + 1] * m[1]) + R[r * 3 + 2] * m[2]);
            if (first == NP) first = k;
            moved++;
        }
        if (moved) LIO_HIP_TRY(hipMemcpy(g->d_priors + first, g->priors.data() + first, (NP - first) * sizeof(PriorDev), hipMemcpyHostToDevice));
    }
    g->moment_open = false;
    return moved;
}

int lio_graph_moment_linearize(lio_graph* g, double bm3[3], double Hmm9[9], double* Hpm, uint32_t node_cap) {
    if (!g) return LIO_E_INVALID;
    if (!g->moment_open) { set_error("lio_graph_moment_linearize: no moment stage is open"); return LIO_E_STATE; }
    const uint32_t N = num_nodes(g);
    if (Hpm && N > node_cap) return LIO_E_CAPACITY;
    int rc = prepare(g);
    if (rc != LIO_OK) return rc;
    rc = launch_linearize(g, -1);
    if (rc == LIO_OK) rc = launch_assemble(g, -1);
    if (rc != LIO_OK) return rc;
    LIO_HIP_TRY(hipStreamSynchronize(g->st));
    if (bm3) LIO_HIP_TRY(hipMemcpy(bm3, g->d_bm, 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (Hmm9) LIO_HIP_TRY(hipMemcpy(Hmm9, g->d_Hmm, 9 * sizeof(double), hipMemcpyDeviceToHost));
    if (Hpm) {
        memset(Hpm, 0, 18ull * N * sizeof(double));
        if (g->Na) {
            std::vector<double> h(18ull * g->Na);
            LIO_HIP_TRY(hipMemcpy(h.data(), g->d_Hpm, h.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (uint32_t a = 0; a < g->Na; a++) memcpy(Hpm + 18ull * g->act[a], &h[18ull * a], 18 * sizeof(double));
        }
    }
    return (int)g->n_mall;
}

int lio_graph_estimate_gnss_moment(lio_graph* g, double max_distance_error, int max_iterations, const double* prior_info9, double moment3[3], lio_graph_report* report) {
    if (!g || !(max_distance_error > 0)) return LIO_E_INVALID;
    if (moment_refuses(g, "lio_graph_estimate_gnss_moment")) return LIO_E_STATE;
    std::vector<uint32_t> gnss;
    for (uint32_t k = 0; k < g->priors.size(); k++) {
        const PriorDev& p = g->priors[k];
        if (!p.live || p.type != LIO_GRAPH_PRIOR_XYZ) continue;
        if (!(max_distance_error * max_distance_error * p.info[0] > 0)) { set_error("lio_graph_estimate_gnss_moment: prior %d has no positive information(0, 0)", p.id); return LIO_E_INVALID; }
        gnss.push_back(k);
    }
    if (moment3) moment3[0] = moment3[1] = moment3[2] = 0.0;
    if (gnss.empty()) return 0;  // nothing to estimate from: nothing is touched
    uint32_t n_live = 1;  // the moment's own prior
    for (uint32_t e = 0; e < num_edges(g); e++) n_live += g->live[e];
    if ((int64_t)n_live < (int64_t)g->par.min_edges) { set_error("lio_graph_estimate_gnss_moment: fewer than min_edges live edges"); return LIO_E_STATE; }
    hipSetDevice(g->device);
    for (uint32_t k : gnss) {
        const int rc = prior_set(g, k, LIO_GRAPH_KERNEL_DCS2, max_distance_error * max_distance_error * g->priors[k].info[0], 1);
        if (rc != LIO_OK) return rc;
    }
    int rc = lio_graph_moment_begin(g, nullptr, prior_info9);
    if (rc != LIO_OK) return rc;
    rc = lio_graph_optimize(g, max_iterations, report);
    if (rc < 0) { lio_graph_moment_end(g, 0); return rc == -1 ? LIO_E_STATE : rc; }
    if (moment3) {
        rc = lio_graph_moment_get(g, moment3);
        if (rc != LIO_OK) { lio_graph_moment_end(g, 0); return rc; }
    }
    return lio_graph_moment_end(g, 1);
}

int lio_graph_last_times(lio_graph* g, double* linearize_us, double* assemble_us, double* solve_us, double* update_us) {
    if (!g) return LIO_E_INVALID;
    if (linearize_us) *linearize_us = g->t_lin;
    if (assemble_us) *assemble_us = g->t_asm;
    if (solve_us) *solve_us = g->t_solve;
    if (update_us) *update_us = g->t_update;
    return LIO_OK;
}

}  // extern "C"
