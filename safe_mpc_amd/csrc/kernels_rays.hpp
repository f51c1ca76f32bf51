// kernels_rays.hpp -- the bookkeeping of safe-set ray labelling on the device (smpc_ray_update): after a round of smpc_sqp_batch and
// smpc_check_guess, one look at every ray in flight -- is its trial pending, feasible or infeasible -- and what follows from it: the
// certificate, the bracket, the ray's end or its next trial.  The statement it follows is safe_set_data.py::ray_update_statement.
#pragma once
#include "kernels_sqp.hpp"

namespace smpc {

// One wavefront per ray.  The decision is a handful of scalars; the work is the scan of the ray's iterate ((N + 1) nx + N nu doubles:
// NaN anywhere, the terminal velocity's largest magnitude and node 0's distance from x0 as lane reductions) and, where the trial is
// resolved, the copy of the iterate into the certificate and the refill with the next trial's constant guess.  Every lane reads an
// element before it writes it and no other lane touches that element, so the two passes need no barrier.  The ray's scalars (the
// SQP state's iters / status / done, the ray's trial / s / lo / hi / open) are read by all 64 lanes before the copy loops and
// overwritten by lane 0 alone after them: the block is exactly one wavefront, which runs in lockstep, so every lane's read precedes
// lane 0's write in program order.  Every branch between the two passes is uniform over the wavefront.
// A ray whose `open` byte is 0 (finished) and a ray whose trial is pending are left untouched, bit for bit.  Nothing is summed
// across rays; *n_open (zeroed by the caller) counts the rays still open with one integer atomic per open ray.
__global__ __launch_bounds__(64) void k_ray_update(int B, int nq, int N, smpc_ray_opts o, smpc_ray_state R, smpc_sqp_state S,
                                                   const int32_t* __restrict__ flags, double* __restrict__ x0,
                                                   double* __restrict__ x_guess, double* __restrict__ u_guess,
                                                   int32_t* __restrict__ n_open) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    if (!R.open[b]) return;
    const int nx = 2 * nq, nX = (N + 1) * nx, nU = N * nq;
    double* const xb = x_guess + (size_t)b * nX;
    double* const ub = u_guess + (size_t)b * nU;
    double* const x0b = x0 + (size_t)b * nx;
    // ---- the look ------------------------------------------------------------------------------------------------------------
    bool bad = false;
    double vmax = 0.0, off = 0.0;
    for (int i = lane; i < nX; i += 64) {
        const double v = xb[i];
        bad = bad || v != v;
        if (i < nx) {
            const double e = v - x0b[i];
            bad = bad || e != e;
            off = fmax(off, fabs(e));
        }
        if (i >= N * nx + nq) vmax = fmax(vmax, fabs(v));
    }
    for (int i = lane; i < nU; i += 64) {
        const double v = ub[i];
        bad = bad || v != v;
    }
    vmax = sqp_wave_max(vmax);
    off = sqp_wave_max(off);
    const bool nan_any = __any(bad) != 0;
    const int32_t it = S.iters[b];
    const bool feasible = S.status[b] == 0 && flags[b] == 0 && vmax <= o.tol_term && off <= 1e-12 && !nan_any;
    const bool ended = S.done[b] != 0 || it >= o.budget || nan_any;
    if (!feasible && !ended) {                       // pending
        if (lane == 0) atomicAdd(n_open, 1);
        return;
    }
    // ---- the trial is resolved: bracket, then the ray's end or its next trial --------------------------------------------------
    const int t = R.trial[b];
    const double s = R.s[b];
    const double lo = feasible ? s : R.lo[b];
    const double hi = feasible ? R.hi[b] : s;
    int kind = SMPC_RAY_OPEN;
    if (!feasible && t == 0) kind = SMPC_RAY_DEAD;
    else if (feasible && t == 1) kind = SMPC_RAY_SATURATED;
    else if (t >= o.bisect + 1) kind = SMPC_RAY_BRACKETED;
    const bool next = kind == SMPC_RAY_OPEN;
    const double s_new = t == 0 ? hi : 0.5 * (lo + hi);
    const double* const qb = R.q + (size_t)b * nq;
    const double* const db = R.d + (size_t)b * nq;
    double* const xc = R.x_cert + (size_t)b * nX;
    double* const uc = R.u_cert + (size_t)b * nU;
    for (int i = lane; i < nX; i += 64) {
        if (feasible) xc[i] = xb[i];
        if (next) {
            const int j = i % nx;
            const double v = j < nq ? qb[j] : s_new * db[j - nq];
            xb[i] = v;
            if (i < nx) x0b[i] = v;
        }
    }
    for (int i = lane; i < nU; i += 64) {
        if (feasible) uc[i] = ub[i];
        if (next) ub[i] = 0.0;
    }
    if (lane != 0) return;
    R.lo[b] = lo;
    R.hi[b] = hi;
    R.trial[b] = t + 1;
    R.iters_total[b] += it;
    if (next) {
        R.s[b] = s_new;
        S.mu[b] = o.mu0;
        S.done[b] = 0;
        S.status[b] = 0;
        S.alpha[b] = 0.0;
        S.merit_before[b] = 0.0;
        S.merit[b] = 0.0;
        S.violation[b] = 0.0;
        S.updated[b] = 0;
        S.iters[b] = 0;
        S.qp_iter_total[b] = 0;
        atomicAdd(n_open, 1);
    } else {
        R.kind[b] = kind;
        R.open[b] = 0;
        S.done[b] = 1;
    }
}

}  // namespace smpc
