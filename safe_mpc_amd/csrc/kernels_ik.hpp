// kernels_ik.hpp -- multi-start inverse kinematics with collision rows on the device (smpc_ik_batch): a joint configuration whose
// end-effector point sits at a target, inside the joint box and clear of every collision row -- the problem of the reference's
// InverseKinematicsOCP (ocp.py:321-326), which hands it to IPOPT one instance at a time.  The statement the kernel follows, step
// for step, is safe_mpc_amd/ik.py::ik_batch_host.
#pragma once
#include "device_model.hpp"

namespace smpc {

constexpr int IK_MAX_STARTS = 64;

// index of (i, j), i >= j, in a packed lower triangle
__host__ __device__ constexpr int ik_tri(int i, int j) { return i * (i + 1) / 2 + j; }

// k_ik keeps the code it had before row_value and point_world existed -- ik_point and ik_row below, a copy of the row switch: through
// the shared statements the 7-DoF instantiation came out measurably slower (profiles/device_model_refactor.txt, section 4), and a
// kernel that does not keep its time keeps its code.  A sixth row kind, or a change to a row's expression, has to be made here as
// well as in row_value.
// world position of a robot point, with its Jacobian columns when ND = NQ (point_with_jacobian) and without when ND = 0
template <int NQ, int ND>
__device__ __forceinline__ DV3<ND> ik_point(const smpc_point& P, const Mat3<double>* Rw, const Vec3<double>* pw, const Vec3<double>* zw) {
    if constexpr (ND > 0) {
        return point_with_jacobian<NQ>(P, Rw, pw, zw);
    } else {
        DV3<0> out = dv_const<0>(P.local);
        if (P.link < 0) return out;
        const Vec3<double> w = pw[P.link] + mulc(Rw[P.link], P.local);
        out.x.v = w.x; out.y.v = w.y; out.z.v = w.z;
        return out;
    }
}

// value (and, ND = NQ, gradient) of one collision row: the expressions of node_geometry (kernels_nodes.hpp)
template <int NQ, int ND, bool SCENE>
__device__ __forceinline__ DQ<ND> ik_row(const smpc_problem_desc* __restrict__ D, const smpc_row& row, const RowGeom<SCENE>& G,
                                         const Mat3<double>* Rw, const Vec3<double>* pw, const Vec3<double>* zw) {
    auto pt = [&](int i) { return ik_point<NQ, ND>(D->points[i], Rw, pw, zw); };
    switch (row.kind) {
    case SMPC_ROW_SEG_FIXEDSEG: return segment_dist2<ND>(pt(row.pa), pt(row.pb), dv_const<ND>(G.C), dv_const<ND>(G.D));
    case SMPC_ROW_SEG_SEG: return segment_dist2<ND>(pt(row.pa), pt(row.pb), pt(row.pc), pt(row.pd));
    case SMPC_ROW_SEG_POINT: return ball_segment_dist2<ND>(pt(row.pa), pt(row.pb), row.len2, dv_const<ND>(G.C));
    case SMPC_ROW_POINT_POINT: {
        DV3<ND> w = pt(row.pa) - dv_const<ND>(G.C);
        return dot(w, w);
    }
    default: {
        DV3<ND> P = pt(row.pa);
        DQ<ND> v = row.axis == 0 ? P.x : (row.axis == 1 ? P.y : P.z);
        v.v -= *G.offset;
        return v;
    }
    }
}

// The stacked residual r(q) of one start: ee(q) - target, then w (lb' - v) / w (v - ub') of the rows beyond their pushed bounds
// lb' = lb + push |lb|, ub' = ub - push |ub|, w = 1 / max(sqrt|bound|, 1e-3); a bound with |.| >= SMPC_INF is absent.
//   F = |r|^2, ee_inf = |ee - target|_inf, margin = max over the present bounds of (lb - v, v - ub), -inf without one
//   ND = NQ: also g = J^T r and the packed lower triangle A of J^T J, accumulated row by row (the Jacobian is never held)
template <int NQ, int ND, bool SCENE>
__device__ __forceinline__ void ik_eval(const smpc_problem_desc* __restrict__ D, const double* q, const double* __restrict__ tgt,
                                        double push, const double* __restrict__ row_lb, const double* __restrict__ row_ub,
                                        const double* __restrict__ geom_b, double& F, double& ee_inf, double& margin, double* g,
                                        double* A) {
    Mat3<double> Rw[NQ];
    Vec3<double> pw[NQ], zw[NQ];
    fk_world<NQ>(D->joints, q, Rw, pw, zw);
    {
        const DV3<ND> ee = ik_point<NQ, ND>(D->points[D->ee_point], Rw, pw, zw);
        const double ex = ee.x.v - tgt[0], ey = ee.y.v - tgt[1], ez = ee.z.v - tgt[2];
        F = ex * ex + ey * ey + ez * ez;
        ee_inf = nanmax(nanmax(fabs(ex), fabs(ey)), fabs(ez));
        if constexpr (ND > 0) {
#pragma unroll
            for (int i = 0; i < NQ; i++) {
                g[i] = ee.x.d[i] * ex + ee.y.d[i] * ey + ee.z.d[i] * ez;
#pragma unroll
                for (int j = 0; j <= i; j++) A[ik_tri(i, j)] = ee.x.d[i] * ee.x.d[j] + ee.y.d[i] * ee.y.d[j] + ee.z.d[i] * ee.z.d[j];
            }
        }
    }
    margin = NEG_INF;
    const int nrows = D->n_rows;
    for (int r = 0; r < nrows; r++) {
        const smpc_row& row = D->rows[r];
        const DQ<ND> v = ik_row<NQ, ND, SCENE>(D, row, row_geom<SCENE>(row, geom_b, r), Rw, pw, zw);
#pragma unroll
        for (int side = 0; side < 2; side++) {
            const double bound = side == 0 ? row_lb[r] : row_ub[r];
            if (!(fabs(bound) < SMPC_INF)) continue;
            const double sign = side == 0 ? -1.0 : 1.0;     // lower bound: violated below it
            margin = nanmax(margin, sign * (v.v - bound));
            const double bp = bound - sign * push * fabs(bound);
            const double w = 1.0 / fmax(sqrt(fabs(bound)), 1e-3);
            const double res = w * sign * (v.v - bp);
            if (!(res > 0.0)) continue;
            F += res * res;
            if constexpr (ND > 0) {
                const double ws = w * sign;
#pragma unroll
                for (int i = 0; i < NQ; i++) {
                    const double ji = ws * v.d[i];
                    g[i] += ji * res;
#pragma unroll
                    for (int j = 0; j <= i; j++) A[ik_tri(i, j)] += ji * (ws * v.d[j]);
                }
            }
        }
    }
}

// dq = -(A + lam I)^-1 g by a Cholesky factorisation in registers (pivots floored at 1e-30: A is positive semi-definite and
// lam >= damping_min > 0, the floor only keeps a rounded-away pivot from producing a NaN)
template <int NQ> __device__ __forceinline__ void ik_solve(const double* A, const double* g, double lam, double* dq) {
    double L[NQ * (NQ + 1) / 2];
#pragma unroll
    for (int j = 0; j < NQ; j++) {
        double d = A[ik_tri(j, j)] + lam;
#pragma unroll
        for (int k = 0; k < j; k++) d -= L[ik_tri(j, k)] * L[ik_tri(j, k)];
        d = d > 1e-30 ? d : 1e-30;
        const double piv = sqrt(d), inv = 1.0 / piv;
        L[ik_tri(j, j)] = piv;
#pragma unroll
        for (int i = j + 1; i < NQ; i++) {
            double s = A[ik_tri(i, j)];
#pragma unroll
            for (int k = 0; k < j; k++) s -= L[ik_tri(i, k)] * L[ik_tri(j, k)];
            L[ik_tri(i, j)] = s * inv;
        }
    }
    double y[NQ];
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        double s = -g[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[ik_tri(i, k)] * y[k];
        y[i] = s / L[ik_tri(i, i)];
    }
#pragma unroll
    for (int i = NQ - 1; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < NQ; k++) s -= L[ik_tri(k, i)] * dq[k];
        dq[i] = s / L[ik_tri(i, i)];
    }
}

// ---- k_ik: S starts of a projected Levenberg-Marquardt iteration per instance ------------------------------------------------------
// One wavefront per instance, lane s = start s (S <= 64; the lanes s >= S idle).  A lane keeps q, the damping, F, J^T r and the
// lower triangle of J^T J in registers and runs exactly max_iter iterations: linearise where the last step was accepted (forward
// tangents, DQ<NQ>), solve, clip to the box, evaluate the trial point forward-only, accept where F fell.  Lanes do not talk until
// the end: a final forward-only evaluation gives each lane's |ee - target|_inf, worst row margin and F, a ballot finds the
// successful lane with the lowest index, and without one a fixed-order butterfly over (F, lane) finds the least F (NaN counts as
// +inf, ties go to the lowest lane).  The winner's lane writes q_out[b], info[b] = {its index, number of successful starts} and
// resid[b] = {|ee - target|_inf, margin}.  No atomics, no LDS, nothing depends on B or on another instance.
// Instances whose mask byte is 0 are skipped and their outputs left as they are.
// SCENE: the rows' fixed obstacles from the scene track sc, column scene_col(time), instead of the descriptor.
template <int NQ, bool SCENE = false>
__global__ __launch_bounds__(64) void k_ik(const smpc_problem_desc* __restrict__ D, int B, int S, const double* __restrict__ target,
                                           const double* __restrict__ q_start, int max_iter, double tol_ee, double push, double lam0,
                                           double lam_accept, double lam_reject, double lam_min, double lam_max,
                                           const double* __restrict__ q_lo, const double* __restrict__ q_hi,
                                           const double* __restrict__ row_lb, const double* __restrict__ row_ub,
                                           const uint8_t* __restrict__ mask, double* __restrict__ q_out, int32_t* __restrict__ info,
                                           double* __restrict__ resid, const SceneArg<SCENE> sc = {}) {
    constexpr int NT = NQ * (NQ + 1) / 2;
    const int b = blockIdx.x, s = threadIdx.x;
    if (b >= B) return;
    if (mask && !mask[b]) return;              // (the same for every lane of the block)
    const bool live = s < S;
    const double* const tgt = target + (size_t)b * 3;
    const double* geom_b = nullptr;
    if constexpr (SCENE) geom_b = scene_block(sc, b, scene_time(sc), D->n_rows);
    double q[NQ];
    double F = POS_INF, ee_inf = POS_INF, margin = POS_INF;
    if (live) {
        const double* qs = q_start + ((size_t)b * S + s) * NQ;
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            const double v = qs[i];
            q[i] = (fabs(v) < POS_INF) ? fmin(fmax(v, q_lo[i]), q_hi[i]) : 0.5 * (q_lo[i] + q_hi[i]);   // (a NaN fails the test)
        }
        double g[NQ], A[NT];
        double lam = lam0;
        bool lin = true;
        for (int it = 0; it < max_iter; it++) {
            if (lin) ik_eval<NQ, NQ, SCENE>(D, q, tgt, push, row_lb, row_ub, geom_b, F, ee_inf, margin, g, A);
            double dq[NQ], qn[NQ];
            ik_solve<NQ>(A, g, lam, dq);
            bool finite = true;
#pragma unroll
            for (int i = 0; i < NQ; i++) {
                const double v = q[i] + dq[i];
                finite = finite && (fabs(v) < POS_INF);
                qn[i] = fmin(fmax(v, q_lo[i]), q_hi[i]);
            }
            double Fn = POS_INF, en, mn;
            if (finite) ik_eval<NQ, 0, SCENE>(D, qn, tgt, push, row_lb, row_ub, geom_b, Fn, en, mn, nullptr, nullptr);
            const bool acc = finite && (Fn < F);
            if (acc) {
#pragma unroll
                for (int i = 0; i < NQ; i++) q[i] = qn[i];
                lam = fmax(lam * lam_accept, lam_min);
            } else {
                lam = fmin(lam * lam_reject, lam_max);
            }
            lin = acc;
        }
        ik_eval<NQ, 0, SCENE>(D, q, tgt, push, row_lb, row_ub, geom_b, F, ee_inf, margin, nullptr, nullptr);
    }
    const bool ok = live && (ee_inf <= tol_ee) && (margin <= 0.0);
    const unsigned long long okm = __ballot(ok);
    int win;
    if (okm) {
        win = __ffsll((long long)okm) - 1;
    } else {
        double bf = (live && F == F) ? F : POS_INF;
        int bi = s;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double of = __shfl_xor(bf, o);
            const int oi = __shfl_xor(bi, o);
            if (of < bf || (of == bf && oi < bi)) { bf = of; bi = oi; }
        }
        win = bi < S ? bi : 0;      // (every F infinite: lane 0, the lowest index)
    }
    if (s != win) return;
    double* qo = q_out + (size_t)b * NQ;
#pragma unroll
    for (int i = 0; i < NQ; i++) qo[i] = q[i];
    info[2 * b] = win;
    info[2 * b + 1] = (int32_t)__popcll(okm);
    resid[2 * b] = ee_inf;
    resid[2 * b + 1] = margin;
}

}  // namespace smpc
