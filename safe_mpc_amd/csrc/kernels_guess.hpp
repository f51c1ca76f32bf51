// kernels_guess.hpp -- the acceptance test of a warm start on the device (smpc_check_guess): AbstractController.checkGuess'
// five predicates per instance as one forward-only kernel, so that a device-resident SQP batch can be asked "who is acceptable
// now" between two calls of smpc_sqp_batch.  The statement it follows is controller.py::checkGuess (env_model.py:170-243,
// safe_set.py:61-68 of the reference).
#pragma once
#include "device_model.hpp"

namespace smpc {

constexpr int GUESS_N_WORST = 5;

// The safe-set node of the instances whose mask byte is set: idx[m] = node (what the network pass reads, mode 3 of run_mlp),
// pos[b] = m (where k_check_guess finds the instance's output).  The order of the list is whatever the atomics give; a row's
// output does not depend on its place in the list.
__global__ void k_guess_nn_list(int B, int N, int safe_node, const uint8_t* __restrict__ mask, int32_t* __restrict__ idx,
                                int32_t* __restrict__ pos, int32_t* __restrict__ m_live) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (mask && !mask[b]) return;
    const int m = atomicAdd(m_live, 1);
    idx[m] = (int32_t)((long)b * (N + 1) + safe_node);
    pos[b] = m;
}

// ---- k_check_guess: the five predicates of checkGuess for B trajectories, forward-only ------------------------------------------
// One wavefront per instance, lane k = node k (N + 1 <= 64).  First the lanes i < NQ roll the double integrator of joint i out from
// node 0 with k_guess_correction's expression order into LDS (x_sim has the bits smpc_guess_correction would write); then lane k
// evaluates its node -- the state box, forward kinematics once for the collision rows (the points' world positions pass through an
// LDS column of the lane's own), the forward-only inverse dynamics for the torque box, the squared distance of node k to x_sim --
// and keeps four partial results in registers.  NaN-keeping maxima and a fixed-order butterfly sum reduce them over the wavefront;
// the safe-set value comes from the network pass's output.  Lane 0 writes worst[b][5] and flags[b]: bit i is set when predicate i
// does NOT pass, and every test is written as "not (passes)", so a NaN fails.  Nothing per node is written.
//   worst[0]  max over nodes and components of max(x_min - x, x - x_max)                        passes when <= tol_x
//   worst[1]  max over the tested nodes' rows of max(lb - v, v - ub); -inf if nothing is tested  passes when <= 0
//             (node 0 only when coll_first != 0, every node otherwise; v as k_merit forms the rows)
//   worst[2]  max over nodes 0..N-1 of max(tau_min - tau, tau - tau_max)                        passes when <= tol_tau
//   worst[3]  |x - x_sim|_2 over the whole trajectory                                            passes when < tol_dyn sqrt(N + 1)
//   worst[4]  -g at node safe_node, g as k_check_nn forms it; -inf and bit clear if safe_node < 0
//                                                                        passes when g >= -tol_safe && g <= 1e6 + tol_safe
// Instances whose mask byte is 0 are skipped and their outputs left as they are.
// SCENE: the rows' fixed obstacles from the scene track sc (node k in column scene_col(time + k)) instead of the descriptor.
// MODEL: the torque margin's link inertials from instance b's own records (md, smpc_set_instance_models) instead of the descriptor's.
template <int NQ, bool SCENE = false, bool MODEL = false, class... MJ>
__global__ __launch_bounds__(64) void k_check_guess(const smpc_problem_desc* __restrict__ D, int B, int N, const double* __restrict__ xg,
                                                    const double* __restrict__ ug, double tol_x, double tol_tau, double tol_dyn,
                                                    double tol_safe, double alpha, int coll_first, int safe_node,
                                                    const double* __restrict__ x_min, const double* __restrict__ x_max,
                                                    const double* __restrict__ tau_min, const double* __restrict__ tau_max,
                                                    const double* __restrict__ row_lb, const double* __restrict__ row_ub,
                                                    const uint8_t* __restrict__ mask, const float* __restrict__ y,
                                                    const int32_t* __restrict__ pos, int32_t* __restrict__ flags,
                                                    double* __restrict__ worst, const SceneArg<SCENE> sc = {},
                                                    const MJ* __restrict__... md) {
    static_assert(ModelArg<MODEL, MJ...>, "md: the table of smpc_joint records when MODEL is set, nothing otherwise");
    constexpr int NX = 2 * NQ;
    __shared__ double s_pts[PT_COL_DOUBLES];
    __shared__ double s_sim[(SMPC_MAX_N + 1) * NX];
    const int b = blockIdx.x, k = threadIdx.x;
    if (b >= B) return;
    if (mask && !mask[b]) return;              // (the same for every lane of the block)
    const double* xb = xg + (long)b * (N + 1) * NX;
    const double* ub = ug + (long)b * N * NQ;
    if (k < NQ) {
        const double dt = D->dt, c = 0.5 * dt * dt;
        double q = xb[k], v = xb[NQ + k];
        s_sim[k] = q;
        s_sim[NQ + k] = v;
        for (int n = 0; n < N; n++) {
            const double un = ub[n * NQ + k];
            q = q + dt * v + c * un;
            v = v + dt * un;
            s_sim[(n + 1) * NX + k] = q;
            s_sim[(n + 1) * NX + NQ + k] = v;
        }
    }
    __syncthreads();
    double w_box = NEG_INF, w_row = NEG_INF, w_tau = NEG_INF, d2 = 0.0;
    if (k <= N) {
        const double* xk = xb + k * NX;
        double q[NQ], v[NQ];
#pragma unroll
        for (int i = 0; i < NQ; i++) {
            q[i] = xk[i];
            v[i] = xk[NQ + i];
            const double eq = q[i] - s_sim[k * NX + i], ev = v[i] - s_sim[k * NX + NQ + i];
            d2 += eq * eq + ev * ev;
        }
        w_box = box_margin<NQ>(q, v, x_min, x_max);
        const int nrows = D->n_rows;
        if (nrows > 0 && (k == 0 || !coll_first)) {
            // forward kinematics: the points' world positions into this lane's LDS column
            double* const spt = s_pts + k;
            point_column_fixed(D, spt);
            point_column_fk<NQ>(D, q, spt);
            const double* geom_b = nullptr;
            if constexpr (SCENE) geom_b = scene_block(sc, b, scene_time(sc) + k, nrows);
            for (int r = 0; r < nrows; r++) {
                const double rv = row_value<0, SCENE>(D->rows[r], row_geom<SCENE>(D->rows[r], geom_b, r), [&](int i) { return column_point(spt, i); }).v;
                w_row = nanmax(w_row, nanmax(row_lb[r] - rv, rv - row_ub[r]));
            }
        }
        if (k < N) {
            const double* uk = ub + k * NQ;
            double u[NQ], tau[NQ];
#pragma unroll
            for (int i = 0; i < NQ; i++) u[i] = uk[i];
            rnea_world<NQ, double>(model_joints<NQ>(D, b, md...), D->gravity, q, v, u, tau);
#pragma unroll
            for (int i = 0; i < NQ; i++) w_tau = nanmax(w_tau, nanmax(tau_min[i] - tau[i], tau[i] - tau_max[i]));
        }
    }
    w_box = wave_nanmax(w_box);
    w_row = wave_nanmax(w_row);
    w_tau = wave_nanmax(w_tau);
    d2 = wave_sum(d2);
    if (k != 0) return;
    const double w_dyn = sqrt(d2);
    double w_safe = NEG_INF;
    int32_t f = 0;
    if (!(w_box <= tol_x)) f |= 1;
    if (!(w_row <= 0.0)) f |= 2;
    if (!(w_tau <= tol_tau)) f |= 4;
    if (!(w_dyn < tol_dyn * sqrt((double)(N + 1)))) f |= 8;
    if (safe_node >= 0) {
        // safe_set.py:61-68, the expression of k_check_nn
        const double* xs = xb + safe_node * NX;
        const double vn2 = safe_speed2<NQ>(D, xs + NQ);
        const double g = safe_value((double)y[pos[b]], alpha, vn2);
        w_safe = -g;
        if (!((g >= -tol_safe) && (g <= 1e6 + tol_safe))) f |= 16;
    }
    double* wb = worst + (long)b * GUESS_N_WORST;
    wb[0] = w_box;
    wb[1] = w_row;
    wb[2] = w_tau;
    wb[3] = w_dyn;
    wb[4] = w_safe;
    flags[b] = f;
}

}  // namespace smpc
