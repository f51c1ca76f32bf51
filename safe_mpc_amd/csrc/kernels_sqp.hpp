// kernels_sqp.hpp -- SQP with merit backtracking on the device (smpc_sqp_batch, smpc_merit_terms): the l1 merit function's two
// terms per instance as one forward-only kernel, and the small kernels of the iteration around it (step, penalty, Armijo update,
// commit).  The statement they follow is closed_loop.py::merit_terms / generate_guess.
#pragma once
#include "device_model.hpp"

namespace smpc {

// x + a d with the product rounded before the sum, as the host statement's numpy expression rounds it (the build contracts
// a * d + x into one fma otherwise): the trial point is then the same number wherever it is formed -- in k_merit, in the list of
// points the network pass reads, in the commit of the accepted iterate.
__device__ __forceinline__ double sqp_axpy(double x, double a, double d) {
#pragma clang fp contract(off)
    return x + a * d;
}

// the acceptance inequality of the line search, rounded operation by operation like the host statement
__device__ __forceinline__ bool sqp_armijo_ok(double merit, double m0, double D, double a, double armijo) {
#pragma clang fp contract(off)
    return merit <= m0 + armijo * a * fmin(D, 0.0) + 1e-12 * (1.0 + fabs(m0));
}

// (kernels_rays.hpp reduces with this name; the reduction itself is device_model.hpp's.  An alias to retire when that header is
//  next edited.)
__device__ __forceinline__ double sqp_wave_max(double v) { return wave_max(v); }

// k_merit and k_score_seg (kernels_score.hpp) keep the code they had before row_value and point_column_fk existed -- this copy of the
// row switch over the LDS column, and their own joint walks: through the shared statements both came out measurably slower
// (profiles/device_model_refactor.txt, section 4), and a kernel that does not keep its time keeps its code.  A sixth row kind, or a
// change to a row's expression, has to be made here as well as in row_value.
// value of one collision row from the points' world positions (env_model.py:263-316; the values k_check_nodes tests); the
// fixed obstacle from the descriptor (G = row_geom<false>) or from the instance's scene (row_geom<true>)
template <bool SCENE>
__device__ __forceinline__ double sqp_row_value(const smpc_row& row, const double* __restrict__ spt, const RowGeom<SCENE>& G) {
    switch (row.kind) {
    case SMPC_ROW_SEG_FIXEDSEG:
        return segment_dist2<0>(column_point(spt, row.pa), column_point(spt, row.pb), dv_const<0>(G.C), dv_const<0>(G.D)).v;
    case SMPC_ROW_SEG_SEG:
        return segment_dist2<0>(column_point(spt, row.pa), column_point(spt, row.pb), column_point(spt, row.pc), column_point(spt, row.pd)).v;
    case SMPC_ROW_SEG_POINT:
        return ball_segment_dist2<0>(column_point(spt, row.pa), column_point(spt, row.pb), row.len2, dv_const<0>(G.C)).v;
    case SMPC_ROW_POINT_POINT: {
        DV3<0> w = column_point(spt, row.pa) - dv_const<0>(G.C);
        return dot(w, w).v;
    }
    default: {
        DV3<0> P = column_point(spt, row.pa);
        return (row.axis == 0 ? P.x.v : (row.axis == 1 ? P.y.v : P.z.v)) - *G.offset;
    }
    }
}

// The nodes whose safe-set row enters the merit function, of the instances whose mask byte is set: the end node (terminal = 1) or
// nodes 1..N, where the node's switch p[4] is on.  idx[m] = node (what the network pass reads, mode 3 of run_mlp), pos[node] = m
// (where k_merit finds the node's output).  The order of the list is whatever the atomics give; no result depends on it.
__global__ void k_sqp_nn_list(int B, int N, int terminal, const double* __restrict__ p, const uint8_t* __restrict__ mask,
                              int32_t* __restrict__ idx, int32_t* __restrict__ pos, int32_t* __restrict__ m_live) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)B * (N + 1)) return;
    const long b = t / (N + 1);
    const int k = (int)(t - b * (N + 1));
    if (k == 0 || (terminal && k != N)) return;
    if (mask && !mask[b]) return;
    if (!(p[t * SMPC_NP + 4] > 0.0)) return;
    const int m = atomicAdd(m_live, 1);
    idx[m] = (int32_t)t;
    pos[t] = m;
}

// the states of the trial points x + a_b dx of the instances whose mask byte is set (what the network pass reads)
__global__ void k_sqp_trial_states(int B, int per, const double* __restrict__ x, const double* __restrict__ dx,
                                   const double* __restrict__ alpha, const uint8_t* __restrict__ mask, double* __restrict__ xt) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)B * per) return;
    const long b = t / per;
    if (mask && !mask[b]) return;
    const double a = alpha ? alpha[b] : 0.0;
    xt[t] = a != 0.0 ? sqp_axpy(x[t], a, dx[t]) : x[t];
}

// ---- k_merit: cost and l1 constraint violation of B trajectories, forward-only ----------------------------------------------------
// One wavefront per instance, lane k = node k (N + 1 <= 64): the lane evaluates its node at the trial point
// (x + a_b dx, u + a_b du) -- forward kinematics once for the EE cost and the collision rows, the forward-only inverse dynamics
// for the torque row, the dynamics defect towards node k + 1, the state box, the safe-set row from the network pass's output --
// and keeps three partial sums in registers (the robot points' world positions pass through an LDS column of the lane's own); a fixed-order butterfly adds them over the wavefront and lane 0 writes
// out[b] = {f, viol, gd}.  Nothing per node is written.  gd = grad f . (dx, du) is formed at a_b = 0 only, from the EE point's
// geometric Jacobian columns (which the forward kinematics has already paid for) against the lane's dq.
// Instances whose mask byte is 0 are skipped and their outputs left as they are.
// SCENE: the rows' fixed obstacles from the scene track sc (node k in column scene_col(time + k)) instead of the descriptor.
// MODEL: the torque term's link inertials from instance b's own records (md, smpc_set_instance_models) instead of the descriptor's.
// A pack that ends in the table of smpc_set_instance_row_bounds (RowBounds, device_model.hpp): the rows' l1 violation at node k is
// taken against entry (b, k, r) of it instead of the descriptor's bounds.
template <int NQ, bool SCENE = false, bool MODEL = false, class... MJ>
__global__ __launch_bounds__(64) void k_merit(const smpc_problem_desc* __restrict__ D, int B, int N, const double* __restrict__ x0,
                                              const double* __restrict__ xg, const double* __restrict__ ug, const double* __restrict__ p,
                                              const double* __restrict__ dxg, const double* __restrict__ dug,
                                              const double* __restrict__ alpha, const uint8_t* __restrict__ mask,
                                              const float* __restrict__ y, const int32_t* __restrict__ pos, double* __restrict__ out,
                                              const SceneArg<SCENE> sc = {}, const MJ* __restrict__... md) {
    static_assert(ModelRowArg<MODEL, MJ...>, "md: the table of smpc_joint records when MODEL is set, then the row-bounds table or nothing");
    constexpr int NX = 2 * NQ;
    __shared__ double s_pts[PT_COL_DOUBLES];
    const int b = blockIdx.x, k = threadIdx.x;
    if (b >= B) return;
    if (mask && !mask[b]) return;
    const double a = (dxg && alpha) ? alpha[b] : 0.0;
    const bool moved = a != 0.0;                 // (a = 0: the point is (x, u) itself, whatever the step holds)
    const bool want_gd = dxg != nullptr && !moved;
    double f = 0.0, viol = 0.0, gd = 0.0;
    if (k <= N) {
        const long node = (long)b * (N + 1) + k;
        const double* xk = xg + node * NX;
        const double* dxk = dxg ? dxg + node * NX : nullptr;
        const double* pk = p + node * SMPC_NP;
        double q[NQ], v[NQ];
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            q[i] = moved ? sqp_axpy(xk[i], a, dxk[i]) : xk[i];
            v[i] = moved ? sqp_axpy(xk[NQ + i], a, dxk[NQ + i]) : xk[NQ + i];
        }
        const double cs = k == N ? D->cost_scale_term : D->cost_scale_stage;
        const bool cost = D->cost_kind != SMPC_COST_ZERO;
        // forward kinematics: joint origins and axes in registers, the points' world positions into this lane's LDS column
        double* const spt = s_pts + k;
        Vec3<double> pw[NQ], zw[NQ];
        {
            const int np = D->n_points;
            for (int pt = 0; pt < np; pt++)
                if (D->points[pt].link < 0) {
#pragma unroll
                    for (int c = 0; c < 3; c++) spt[(3 * pt + c) * 64] = D->points[pt].local[c];
                }
            Mat3<double> R;
#pragma unroll
            for (int i = 0; i < 9; i++) R.m[i] = (i % 4 == 0) ? 1.0 : 0.0;
            Vec3<double> pc;
#pragma unroll
            for (int i = 0; i < NQ; i++) {
                pc = pc + mulc(R, D->joints[i].p0);
                advance_rotation(R, D->joints[i], q[i]);
                pw[i] = pc;
                zw[i] = mulc(R, D->joints[i].axis);
                for (int pt = 0; pt < np; pt++)
                    if (D->points[pt].link == i) {
                        const Vec3<double> w = pc + mulc(R, D->points[pt].local);
                        spt[(3 * pt) * 64] = w.x;
                        spt[(3 * pt + 1) * 64] = w.y;
                        spt[(3 * pt + 2) * 64] = w.z;
                    }
            }
        }
        if (cost) {
            const int eep = D->ee_point, link = D->points[eep].link;
            const Vec3<double> P(spt[(3 * eep) * 64], spt[(3 * eep + 1) * 64], spt[(3 * eep + 2) * 64]);
            const Vec3<double> del(P.x - pk[0], P.y - pk[1], P.z - pk[2]);
            f += cs * D->Q * dot(del, del);
            if (want_gd) {
                // cost_grad_q[j] = 2 Q (dP/dq_j . del), dP/dq_j = z_j x (P - p_j) for j <= link
                double g = 0.0;
#pragma unroll
                for (int j = 0; j < NQ; j++)
                    if (j <= link) g += 2.0 * D->Q * dot(cross(zw[j], P - pw[j]), del) * dxk[j];
                gd += cs * g;
            }
        }
        if (k == 0) {
            const double* xs = x0 + (long)b * NX;
#pragma unroll
            for (int i = 0; i < NQ; i++) viol += fabs(q[i] - xs[i]) + fabs(v[i] - xs[NQ + i]);
        } else {
            // state box of nodes 1..N
            const double* lo = k == N ? D->x_lo_e : D->x_lo;
            const double* hi = k == N ? D->x_hi_e : D->x_hi;
#pragma unroll
            for (int i = 0; i < NQ; i++) {
                viol += fmax(lo[i] - q[i], 0.0) + fmax(q[i] - hi[i], 0.0);
                viol += fmax(lo[NQ + i] - v[i], 0.0) + fmax(v[i] - hi[NQ + i], 0.0);
            }
            // collision rows of nodes 1..N
            const int nrows = D->n_rows;
            const double* geom_b = nullptr;
            if constexpr (SCENE) geom_b = scene_block(sc, b, scene_time(sc) + k, nrows);
            for (int r = 0; r < nrows; r++) {
                const smpc_row& row = D->rows[r];
                const double rv = sqp_row_value<SCENE>(row, spt, row_geom<SCENE>(row, geom_b, r));
                // (the two branches state one rule on two sources; the descriptor's keeps the very expressions it had, and so its code)
                if constexpr (RowBounds<MJ...>) {
                    const RowLbUb own = row_bounds_at(row_bounds_table(md...), B, N, nrows, b, k, r);
                    if (fabs(own.lb) < SMPC_INF) viol += fmax(own.lb - rv, 0.0);
                    if (fabs(own.ub) < SMPC_INF) viol += fmax(rv - own.ub, 0.0);
                } else {
                    if (fabs(row.lb) < SMPC_INF) viol += fmax(row.lb - rv, 0.0);
                    if (fabs(row.ub) < SMPC_INF) viol += fmax(rv - row.ub, 0.0);
                }
            }
            // safe-set row: max(-g, 0) with g = y (100 - alpha) / 100 - |v| (safe_set.py:94), where the formulation has the row
            const int mode = D->nn_mode;
            if (y && (mode == SMPC_NN_ALL || (mode == SMPC_NN_TERMINAL && k == N)) && pk[4] > 0.0) {
                const int nd = D->nn_dof;
                double vn2 = 0.0;
#pragma unroll
                for (int i = 0; i < NQ; i++) {
                    const double w = i < nd ? v[i] + (i == 0 ? D->nn_eps : 0.0) : 0.0;
                    vn2 += w * w;
                }
                const double g = (double)y[pos[node]] * ((100.0 - pk[3]) / 100.0) - sqrt(vn2);
                viol += fmax(-g, 0.0);
            }
        }
        if (k < N) {
            const double* uk = ug + ((long)b * N + k) * NQ;
            const double* duk = dug ? dug + ((long)b * N + k) * NQ : nullptr;
            const double* xn = xk + NX;             // node k + 1
            const double* dxn = dxk ? dxk + NX : nullptr;
            const double dt = D->dt, c = 0.5 * dt * dt;
            double u[NQ], tau[NQ];
            double uu = 0.0, ud = 0.0;
#pragma unroll
            for (int i = 0; i < NQ; i++) {
                u[i] = moved ? sqp_axpy(uk[i], a, duk[i]) : uk[i];
                uu += u[i] * u[i];
                if (want_gd) ud += u[i] * duk[i];
                // defect of the double integrator towards node k + 1
                const double qn = moved ? sqp_axpy(xn[i], a, dxn[i]) : xn[i];
                const double vn = moved ? sqp_axpy(xn[NQ + i], a, dxn[NQ + i]) : xn[NQ + i];
                viol += fabs(qn - (q[i] + dt * v[i] + c * u[i])) + fabs(vn - (v[i] + dt * u[i]));
            }
            if (cost) {
                f += cs * D->R * uu;
                if (want_gd) gd += cs * 2.0 * D->R * ud;
            }
            rnea_world<NQ, double>(model_joints<NQ>(D, b, md...), D->gravity, q, v, u, tau);
#pragma unroll
            for (int i = 0; i < NQ; i++) viol += fmax(fabs(tau[i]) - D->joints[i].tau_max, 0.0);
        }
    }
    f = wave_sum(f);
    viol = wave_sum(viol);
    gd = wave_sum(gd);
    if (k == 0) {
        out[(long)b * 3] = f;
        out[(long)b * 3 + 1] = viol;
        out[(long)b * 3 + 2] = gd;
    }
}

// ---- the iteration around it ----------------------------------------------------------------------------------------------------
// act[b] = !done[b]: the instances this iteration solves (the QP kernels' and the stage builder's mask)
__global__ void k_sqp_begin(int B, const uint8_t* __restrict__ done, uint8_t* __restrict__ act, int32_t* __restrict__ n_open) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b == 0) *n_open = 0;
    if (b >= B) return;
    act[b] = done[b] ? 0 : 1;
}

// (dx, du) = QP solution - iterate and step[b] = their largest magnitude; one wavefront per active instance
__global__ __launch_bounds__(64) void k_sqp_direction(int B, int nX, int nU, const uint8_t* __restrict__ act, const double* __restrict__ x,
                                                      const double* __restrict__ u, const double* __restrict__ xs,
                                                      const double* __restrict__ us, double* __restrict__ dx, double* __restrict__ du,
                                                      double* __restrict__ step) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B || !act[b]) return;
    double m = 0.0;
    bool bad = false;
    for (int i = lane; i < nX; i += 64) {
        const double d = xs[(long)b * nX + i] - x[(long)b * nX + i];
        dx[(long)b * nX + i] = d;
        bad = bad || d != d;
        m = fmax(m, fabs(d));
    }
    for (int i = lane; i < nU; i += 64) {
        const double d = us[(long)b * nU + i] - u[(long)b * nU + i];
        du[(long)b * nU + i] = d;
        bad = bad || d != d;
        m = fmax(m, fabs(d));
    }
    m = wave_max(m);
    // (numpy's max propagates a NaN, fmax drops it: a step with a NaN in it has no length)
    if (__any(bad)) m = __builtin_nan("");
    if (lane == 0) step[b] = m;
}

// after the merit terms at a = 0: penalty, merit and its directional derivative, the line search's starting state.
// m0t[b] = {f0, c0, gd}.  Also the solve's bookkeeping of the active instances (status, iteration counters).
__global__ void k_sqp_penalty(int B, double mu_max, const uint8_t* __restrict__ act, const int32_t* __restrict__ st,
                              const int32_t* __restrict__ it, const double* __restrict__ m0t, double* __restrict__ mu,
                              double* __restrict__ m0, double* __restrict__ Dd, double* __restrict__ alpha, uint8_t* __restrict__ settled,
                              uint8_t* __restrict__ trial, int32_t* __restrict__ status, int32_t* __restrict__ iters,
                              int32_t* __restrict__ qp_iter_total) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (!act[b]) {
        settled[b] = 1;
        trial[b] = 0;
        return;
    }
    const double f0 = m0t[3 * b], c0 = m0t[3 * b + 1], gd = m0t[3 * b + 2];
    // penalty large enough for  D = grad f . d - mu |c|_1 < 0  wherever the iterate is infeasible
    const double need = c0 > 1e-12 ? 2.0 * fmax(gd, 0.0) / fmax(c0, 1e-12) : 0.0;
    const double m = fmin(fmax(mu[b], need), mu_max);
    mu[b] = m;
    m0[b] = sqp_axpy(f0, m, c0);
    Dd[b] = sqp_axpy(gd, -m, c0);
    alpha[b] = 1.0;
    const bool s = st[b] != 0;
    settled[b] = s;
    trial[b] = !s;
    status[b] = st[b];
    iters[b] += 1;
    qp_iter_total[b] += it[b];
}

// after the merit terms of a trial pass: Armijo test of the instances still searching, next step length or settled
__global__ void k_sqp_armijo(int B, double armijo, double reduction, double alpha_min, const double* __restrict__ mt,
                             const double* __restrict__ mu, const double* __restrict__ m0, const double* __restrict__ Dd,
                             double* __restrict__ alpha, uint8_t* __restrict__ settled, uint8_t* __restrict__ trial) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || settled[b]) return;
    const double a = alpha[b];
    const bool ok = sqp_armijo_ok(sqp_axpy(mt[3 * b], mu[b], mt[3 * b + 1]), m0[b], Dd[b], a, armijo);
    if (ok || a <= alpha_min) {
        settled[b] = 1;
        trial[b] = 0;
    } else {
        alpha[b] = fmax(a * reduction, alpha_min);
    }
}

// the iteration's outcome per active instance: which instances take their step, what the state reports, done, and the count of
// instances still open (integer atomic: one per wavefront)
__global__ void k_sqp_finish(int B, double tol, const uint8_t* __restrict__ act, const int32_t* __restrict__ st,
                             const double* __restrict__ step, const double* __restrict__ alpha, const double* __restrict__ mu,
                             const double* __restrict__ m0, const double* __restrict__ m0t, const double* __restrict__ mt,
                             uint8_t* __restrict__ done, uint8_t* __restrict__ updated, double* __restrict__ o_alpha,
                             double* __restrict__ o_before, double* __restrict__ o_merit, double* __restrict__ o_viol,
                             int32_t* __restrict__ n_open) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    bool open = false;
    if (b < B) {
        if (act[b]) {
            const bool upd = st[b] == 0;
            const double a = alpha[b];
            updated[b] = upd;
            o_alpha[b] = upd ? a : 0.0;
            o_before[b] = m0[b];
            o_merit[b] = upd ? sqp_axpy(mt[3 * b], mu[b], mt[3 * b + 1]) : m0[b];
            o_viol[b] = upd ? mt[3 * b + 1] : m0t[3 * b + 1];
            const bool d = (a * step[b] < tol) || st[b] != 0;
            done[b] = d;
            open = !d;
        }
    }
    const unsigned long long m = __ballot(open);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_open, (int)__popcll(m));
}

// x += a_b dx, u += a_b du for the instances that take their step (the same rounding as the trial point that was accepted)
__global__ void k_sqp_commit(int B, int nX, int nU, const uint8_t* __restrict__ act, const uint8_t* __restrict__ updated,
                             const double* __restrict__ alpha, const double* __restrict__ dx, const double* __restrict__ du,
                             double* __restrict__ x, double* __restrict__ u) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int per = nX + nU;
    if (t >= (long)B * per) return;
    const long b = t / per;
    const int i = (int)(t - b * per);
    if (!act[b] || !updated[b]) return;
    const double a = alpha[b];
    if (i < nX) x[b * nX + i] = sqp_axpy(x[b * nX + i], a, dx[b * nX + i]);
    else u[b * nU + i - nX] = sqp_axpy(u[b * nU + i - nX], a, du[b * nU + i - nX]);
}

}  // namespace smpc
