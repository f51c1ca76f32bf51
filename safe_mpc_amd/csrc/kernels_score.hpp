// kernels_score.hpp -- scoring a closed-loop run where its logs are (smpc_score_rollout): the closed-loop cost of the reference's
// metric (metrics_count_fails.py:19-28), the distance the convergence test compares with tol_conv (mpc.py:273) and how close the run
// came to the obstacles, the state box (env_model.py:170-172, 236-243) and the learned safe set (safe_set.py:61-68), per instance and
// forward-only.  The statement they follow is closed_loop.py::score_rollout_statement.
#pragma once
#include "device_model.hpp"
#include "kernels_sqp.hpp"      // sqp_row_value: k_score_seg keeps the code it had (see there)

namespace smpc {

constexpr int SCORE_ND = 7;         // doubles per instance: cost, sum |ee - ref|^2, sum |u|^2, |ee - ref| at the last state, the margins
constexpr int SCORE_NI = 4;         // int32 per instance: where the margins were taken
// The steps are cut into segments of SCORE_SEG by ABSOLUTE step index -- segment s holds steps s SCORE_SEG .. (s + 1) SCORE_SEG - 1,
// whatever B and n_steps are -- so that a 300-step log of 4096 instances is 640 wavefronts and not 64.  A compile-time constant: the
// order in which an instance's terms are added (ascending inside a segment, then the segments ascending) is the same in every call.
constexpr int SCORE_SEG = 32;
constexpr int SCORE_PD = 5;         // partial doubles per (segment, instance): s1, s2, |ee - ref|^2 at step last_x, coll margin, box margin
constexpr int SCORE_PI = 3;         // partial int32: step and row of the coll margin, step of the box margin

// "b replaces a" of a running maximum / minimum that keeps the FIRST NaN it sees and, among equal values, the first one
__device__ __forceinline__ bool score_takes_max(double a, double b) { return b > a || (b != b && a == a); }
__device__ __forceinline__ bool score_takes_min(double a, double b) { return b < a || (b != b && a == a); }

// last valid rows of instance b's logs, clamped to the logs (a caller's out-of-range entry must not become an out-of-range load)
__device__ __forceinline__ void score_last_rows(int b, int n_steps, const int64_t* __restrict__ last_x, const int64_t* __restrict__ last_u,
                                                int& lx, int& lu) {
    const long x = last_x ? (long)last_x[b] : (long)n_steps, u = last_u ? (long)last_u[b] : (long)n_steps - 1;
    lx = (int)(x < 0 ? 0 : (x > n_steps ? n_steps : x));
    lu = (int)(u < -1 ? -1 : (u > n_steps - 1 ? n_steps - 1 : u));
}

// ---- k_score_seg: one segment of the steps of 64 instances ----------------------------------------------------------------------
// Lane = instance b = blockIdx.x * 64 + lane, blockIdx.y = segment: the logs are step-major, so the 64 lanes' rows of one step are
// 64 * nx (64 * nu) consecutive doubles and every load of the walk is coalesced; nothing is reduced across lanes.  Per step the lane
// runs the forward kinematics once (the points' world positions pass through an LDS column of the lane's own, as in k_merit: the
// rows name their points by run-time index), adds |ee - ref|^2 and |u|^2 to its two sums and updates the two running maxima with
// their places.  Rows past last_x / last_u are never loaded.  A lane whose log ends before the segment writes nothing
// (k_score_combine does not read that segment's partial).  Partials are stored [segment][slot][B], so the stores coalesce too.
// SCENE: the rows' fixed obstacles from the scene track sc instead of the descriptor: state j of the log in column scene_col(j)
// (the log starts at time 0; the clock is not read).
// traj_stride: instance b's reference table starts at traj + b * traj_stride -- 0 for the shared table, 3 * traj_len for the
// handle's per-instance curves (smpc_set_instance_curves); a run-time argument, so the curves add no instantiation.
template <int NQ, bool SCENE = false>
__global__ __launch_bounds__(64) void k_score_seg(const smpc_problem_desc* __restrict__ D, int B, int n_steps,
                                                  const double* __restrict__ x_log, const double* __restrict__ u_log,
                                                  const int64_t* __restrict__ last_x, const int64_t* __restrict__ last_u,
                                                  const double* __restrict__ x_min, const double* __restrict__ x_max,
                                                  const double* __restrict__ row_lb, const double* __restrict__ row_ub,
                                                  const double* __restrict__ ee_ref, const double* __restrict__ traj, long traj_len,
                                                  long traj_stride, const uint8_t* __restrict__ mask, double* __restrict__ pd,
                                                  int32_t* __restrict__ pi, const SceneArg<SCENE> sc = {}) {
    constexpr int NX = 2 * NQ;
    __shared__ double s_pts[PT_COL_DOUBLES];
    const int b = blockIdx.x * 64 + threadIdx.x, seg = blockIdx.y;
    if (b >= B) return;
    if (mask && !mask[b]) return;
    int lx, lu;
    score_last_rows(b, n_steps, last_x, last_u, lx, lu);
    const int j0 = seg * SCORE_SEG;
    if (lx < j0) return;
    const int j1 = lx < j0 + SCORE_SEG - 1 ? lx : j0 + SCORE_SEG - 1;      // last step of this lane in the segment
    double* const spt = s_pts + threadIdx.x;
    const int np = D->n_points, nrows = D->n_rows, eep = D->ee_point;
    const double* const traj_b = traj ? traj + (size_t)b * traj_stride : nullptr;
    for (int pt = 0; pt < np; pt++)
        if (D->points[pt].link < 0) {
#pragma unroll
            for (int c = 0; c < 3; c++) spt[(3 * pt + c) * 64] = D->points[pt].local[c];
        }
    double s1 = 0.0, s2 = 0.0, e_last = 0.0, m_row = NEG_INF, m_box = NEG_INF;
    int st_row = -1, r_row = -1, st_box = -1;
    for (int j = j0; j <= j1; j++) {
        const double* xj = x_log + ((long)j * B + b) * NX;
        double q[NQ], v[NQ];
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            q[i] = xj[i];
            v[i] = xj[NQ + i];
        }
        // state box: max over the components of max(x_min - x, x - x_max)
        double w = NEG_INF;
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            w = nanmax(w, nanmax(x_min[i] - q[i], q[i] - x_max[i]));
            w = nanmax(w, nanmax(x_min[NQ + i] - v[i], v[i] - x_max[NQ + i]));
        }
        if (score_takes_max(m_box, w)) {
            m_box = w;
            st_box = j;
        }
        // forward kinematics: the points' world positions into this lane's LDS column
        Mat3<double> R;
#pragma unroll
        for (int i = 0; i < 9; i++) R.m[i] = (i % 4 == 0) ? 1.0 : 0.0;
        Vec3<double> pc;
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            pc = pc + mulc(R, D->joints[i].p0);
            advance_rotation(R, D->joints[i], q[i]);
            for (int pt = 0; pt < np; pt++)
                if (D->points[pt].link == i) {
                    const Vec3<double> pw = pc + mulc(R, D->points[pt].local);
                    spt[(3 * pt) * 64] = pw.x;
                    spt[(3 * pt + 1) * 64] = pw.y;
                    spt[(3 * pt + 2) * 64] = pw.z;
                }
        }
        // |ee - ref_j|^2, ref_j = ee_ref or column min(j, traj_len - 1) of traj
        double ref[3];
        if (traj) {
            const long c = j < traj_len - 1 ? (long)j : traj_len - 1;
#pragma unroll
            for (int a = 0; a < 3; a++) ref[a] = traj_b[a * traj_len + c];
        } else {
#pragma unroll
            for (int a = 0; a < 3; a++) ref[a] = ee_ref[a];
        }
        const Vec3<double> del(spt[(3 * eep) * 64] - ref[0], spt[(3 * eep + 1) * 64] - ref[1], spt[(3 * eep + 2) * 64] - ref[2]);
        const double e2 = dot(del, del);
        s1 += e2;
        if (j == lx) e_last = e2;
        // collision rows: max over the rows of max(lb - v, v - ub), rows ascending; state j of the log in the scene of time j
        const double* geom_b = nullptr;
        if constexpr (SCENE) geom_b = scene_block(sc, b, j, nrows);
        for (int r = 0; r < nrows; r++) {
            const double rv = sqp_row_value<SCENE>(D->rows[r], spt, row_geom<SCENE>(D->rows[r], geom_b, r));
            const double m = nanmax(row_lb[r] - rv, rv - row_ub[r]);
            if (score_takes_max(m_row, m)) {
                m_row = m;
                st_row = j;
                r_row = r;
            }
        }
        if (j <= lu) {
            const double* uj = u_log + ((long)j * B + b) * NQ;
            double uu = 0.0;
#pragma unroll
            for (int i = 0; i < NQ; i++) uu += uj[i] * uj[i];
            s2 += uu;
        }
    }
    const long at = (long)seg * SCORE_PD * B + b;
    pd[at] = s1;
    pd[at + B] = s2;
    pd[at + 2L * B] = e_last;
    pd[at + 3L * B] = m_row;
    pd[at + 4L * B] = m_box;
    const long ai = (long)seg * SCORE_PI * B + b;
    pi[ai] = st_row;
    pi[ai + B] = r_row;
    pi[ai + 2L * B] = st_box;
}

// ---- k_score_safe: the running least safe-set value over one pass of the network ---------------------------------------------------
// The network's forward pass runs over the flat rows m = j B + b of the state log in passes of a bounded row count; after the pass
// over rows m0 .. m0 + rows - 1 (outputs y[m - m0]) thread b visits ITS rows of the pass, steps ascending, and carries
// gmin[b] / gstep[b] from pass to pass (first != 0: starts them).  One thread owns an instance in every pass and the passes are
// stream-ordered, so the order is fixed.  g as k_check_nn forms it.
template <int NQ>
__global__ __launch_bounds__(64) void k_score_safe(const smpc_problem_desc* __restrict__ D, int B, int n_steps, long m0, long rows,
                                                   int first, const double* __restrict__ x_log, const int64_t* __restrict__ last_x,
                                                   const int64_t* __restrict__ last_u, double alpha, const uint8_t* __restrict__ mask,
                                                   const float* __restrict__ y, double* __restrict__ gmin, int32_t* __restrict__ gstep) {
    constexpr int NX = 2 * NQ;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    if (mask && !mask[b]) return;
    int lx, lu;
    score_last_rows(b, n_steps, last_x, last_u, lx, lu);
    double best = first ? POS_INF : gmin[b];
    int at = first ? -1 : gstep[b];
    const int nd = D->nn_dof;
    const double eps = D->nn_eps;
    long j = m0 <= b ? 0 : (m0 - b + B - 1) / B;              // first step with j B + b >= m0
    for (; j <= lx && j * B + b < m0 + rows; j++) {
        const long m = j * B + b;
        const double* xj = x_log + m * NX;
        // (safe_speed2 / safe_value of device_model.hpp written out, with nd and eps read before the loop: called from inside
        //  this loop they changed the kernel's gfx950 code, and the kernel is kept as it was)
        double vn2 = 0.0;
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            const double vv = i < nd ? xj[NQ + i] + (i == 0 ? eps : 0.0) : 0.0;
            vn2 += vv * vv;
        }
        const double g = (double)y[m - m0] * (100.0 - alpha) / 100.0 - sqrt(vn2);
        if (score_takes_min(best, g)) {
            best = g;
            at = (int)j;
        }
    }
    gmin[b] = best;
    gstep[b] = at;
}

// ---- k_score_combine: the segments' partials in ascending order -> out[b][SCORE_ND], outi[b][SCORE_NI] -------------------------------
// Thread per instance; reads the segments 0 .. last_x / SCORE_SEG its log reaches (the only ones k_score_seg wrote for it).
__global__ __launch_bounds__(64) void k_score_combine(int B, int n_steps, double Q, double Rw, const int64_t* __restrict__ last_x,
                                                      const int64_t* __restrict__ last_u, const uint8_t* __restrict__ mask,
                                                      const double* __restrict__ pd, const int32_t* __restrict__ pi,
                                                      const double* __restrict__ gmin, const int32_t* __restrict__ gstep,
                                                      double* __restrict__ out, int32_t* __restrict__ outi) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    if (mask && !mask[b]) return;
    int lx, lu;
    score_last_rows(b, n_steps, last_x, last_u, lx, lu);
    const int s_last = lx / SCORE_SEG;
    double s1 = 0.0, s2 = 0.0, e_last = 0.0, m_row = NEG_INF, m_box = NEG_INF;
    int st_row = -1, r_row = -1, st_box = -1;
    for (int s = 0; s <= s_last; s++) {
        const long at = (long)s * SCORE_PD * B + b, ai = (long)s * SCORE_PI * B + b;
        s1 += pd[at];
        s2 += pd[at + B];
        if (s == s_last) e_last = pd[at + 2L * B];
        const double mr = pd[at + 3L * B], mb = pd[at + 4L * B];
        if (score_takes_max(m_row, mr)) {
            m_row = mr;
            st_row = pi[ai];
            r_row = pi[ai + B];
        }
        if (score_takes_max(m_box, mb)) {
            m_box = mb;
            st_box = pi[ai + 2L * B];
        }
    }
    double* o = out + (long)b * SCORE_ND;
    o[0] = Q * s1 + Rw * s2;
    o[1] = s1;
    o[2] = s2;
    o[3] = sqrt(e_last);
    o[4] = m_row;
    o[5] = m_box;
    o[6] = gmin ? gmin[b] : POS_INF;
    int32_t* oi = outi + (long)b * SCORE_NI;
    oi[0] = st_row;
    oi[1] = r_row;
    oi[2] = st_box;
    oi[3] = gmin ? gstep[b] : -1;
}

}  // namespace smpc
