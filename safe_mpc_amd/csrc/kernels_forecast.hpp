// Obstacle forecasts: the horizon's N + 1 scenes formed from what the WORLD track has shown up to the scene
// clock, into the scene slot the solve reads -- a table, not a velocity, so no solve-path kernel changes.
#pragma once
#include "device_model.hpp"
#include "kernels_mlp.hpp"

namespace smpc {

// One 64-byte scene record {C[3], D[3], offset, 0} as four 16-byte pieces: every record of a hipMalloc'ed [..][SMPC_SCENE_ROW] table
// is 64-byte aligned, so the pieces load and store as dwordx4.
struct alignas(16) ScenePiece { double a, b; };
struct SceneRec { ScenePiece q[SMPC_SCENE_ROW / 2]; };
static_assert(sizeof(SceneRec) == sizeof(double) * SMPC_SCENE_ROW, "a scene record is SMPC_SCENE_ROW doubles");

__device__ __forceinline__ SceneRec scene_rec_load(const double* __restrict__ p) {
    const ScenePiece* s = static_cast<const ScenePiece*>(__builtin_assume_aligned(p, 16));
    SceneRec r;
#pragma unroll
    for (int i = 0; i < SMPC_SCENE_ROW / 2; i++) r.q[i] = s[i];
    return r;
}
__device__ __forceinline__ void scene_rec_store(double* __restrict__ p, const SceneRec& r) {
    ScenePiece* s = static_cast<ScenePiece*>(__builtin_assume_aligned(p, 16));
#pragma unroll
    for (int i = 0; i < SMPC_SCENE_ROW / 2; i++) s[i] = r.q[i];
}

// k_scene_forecast: F [B][N+1][n_rows][SMPC_SCENE_ROW] from the world W = world.geom [B][T][n_rows][SMPC_SCENE_ROW].  With t the
// scene clock's cell (scene_time: 0 without one, held to +-2^62) and col = scene_col with W's T, for all eight slots of a record
//   SMPC_FORECAST_HOLD  F[b][k] = W[b][col(t)]
//   SMPC_FORECAST_CV    d = W[b][col(t)] - W[b][col(t - 1)];  F[b][0] = W[b][col(t)],  F[b][k] = F[b][k-1] + d
//   SMPC_FORECAST_TRUE  F[b][k] = W[b][col(t + k)]
// A thread owns one (instance, row) record and walks k = 0..N writing whole records; nothing is shared between threads, so an
// instance's result depends neither on B nor on its neighbours, and two calls give the same bits.  CV is repeated addition in this
// order: one subtraction and N additions per slot and not one multiplication, so -ffp-contract has nothing to fuse and the kernel
// equals problem.forecast_statement bit for bit (the argument k_ray_update makes).  No atomics, no LDS.
template <int MODE>
__global__ __launch_bounds__(64) void k_scene_forecast(int n_rec, int n_rows, int N, SceneSrc world, double* __restrict__ F) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_rec) return;
    const int b = i / n_rows, r = i % n_rows;
    const int64_t t = scene_time(world);
    const size_t rec = (size_t)r * SMPC_SCENE_ROW;
    double* out = F + (size_t)b * (size_t)(N + 1) * n_rows * SMPC_SCENE_ROW + rec;
    const size_t step = (size_t)n_rows * SMPC_SCENE_ROW;
    if constexpr (MODE == SMPC_FORECAST_TRUE) {
        for (int k = 0; k <= N; k++) scene_rec_store(out + k * step, scene_rec_load(scene_block(world, b, t + k, n_rows) + rec));
    } else {
        SceneRec f = scene_rec_load(scene_block(world, b, t, n_rows) + rec);
        SceneRec d;
        if constexpr (MODE == SMPC_FORECAST_CV) {
            d = scene_rec_load(scene_block(world, b, t - 1, n_rows) + rec);
#pragma unroll
            for (int s = 0; s < SMPC_SCENE_ROW / 2; s++) { d.q[s].a = f.q[s].a - d.q[s].a; d.q[s].b = f.q[s].b - d.q[s].b; }
        }
        scene_rec_store(out, f);
        for (int k = 1; k <= N; k++) {
            if constexpr (MODE == SMPC_FORECAST_CV) {
#pragma unroll
                for (int s = 0; s < SMPC_SCENE_ROW / 2; s++) { f.q[s].a = f.q[s].a + d.q[s].a; f.q[s].b = f.q[s].b + d.q[s].b; }
            }
            scene_rec_store(out + k * step, f);
        }
    }
}

// The weights of a least-squares line through m equally spaced samples, ages j = 0..m-1 (j = 0 the newest), for m = 1..SMPC_FIT_MAX:
//   u_j = (4m - 2 - 6j) / (m (m + 1))           the line's value now    is sum u_j y_j
//   w_j = (6(m - 1) - 12j) / (m (m^2 - 1))      its step per column     is sum w_j y_j        (m = 1: w_0 = 0)
// Numerators and denominators are small integers, so every weight is ONE correctly rounded division -- done by the compiler, which
// divides as IEEE 754 says, so the table holds the bits of problem.fit_weights.  Row m starts at m (m - 1) / 2.  In the code
// object's constant data: no upload, and a captured launch carries nothing but its arguments.
struct FitWeights {
    double u[SMPC_FIT_MAX * (SMPC_FIT_MAX + 1) / 2], w[SMPC_FIT_MAX * (SMPC_FIT_MAX + 1) / 2];
    constexpr FitWeights() : u{}, w{} {
        for (int m = 1; m <= SMPC_FIT_MAX; m++)
            for (int j = 0; j < m; j++) {
                u[m * (m - 1) / 2 + j] = (double)(4 * m - 2 - 6 * j) / (double)(m * (m + 1));
                w[m * (m - 1) / 2 + j] = m == 1 ? 0.0 : (double)(6 * (m - 1) - 12 * j) / (double)(m * (m * m - 1));
            }
    }
};
__constant__ constexpr FitWeights FIT_WEIGHTS{};

// a product rounded BEFORE it is summed: the build contracts a * b + c into one fma (-ffp-contract=fast), and `#pragma clang fp
// contract(off)` did not stop it on gfx950; an empty register barrier on the product does (v_mul_f64, then v_add_f64)
__device__ __forceinline__ double rounded_product(double a, double b) {
    double p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

// k_scene_fit: F [B][N+1][n_rows][SMPC_SCENE_ROW] from S = seen.geom [B][T][n_rows][SMPC_SCENE_ROW], what the controller has seen of
// the world (the observed track, or the world itself).  With t the scene clock's cell (scene_time), col = scene_col with S's T,
// m = min(window, max(t, 0) + 1) -- nothing was seen before time 0 -- and y_j = S[b][col(t - j)][r][s], for all eight slots
//   a = u_0 y_0;  a = a + u_j y_j  (j = 1..m-1);   d = w_0 y_0;  d = d + w_j y_j       -- every product rounded before its sum
//   F[b][0] = a,  F[b][k] = F[b][k-1] + d                                              -- repeated addition, as SMPC_FORECAST_CV
// which is problem.fit_forecast_statement operation for operation, so the kernel equals it bit for bit; window 1 is HOLD and
// window 2 (u = (1, 0), w = (1, -1)) is SMPC_FORECAST_CV.
// A thread owns ONE 16-byte piece of a record, so four neighbouring lanes load and store a whole 64-byte record and a wavefront's
// access covers 16 whole records (k_scene_forecast's thread owns a record: four accesses of 16 bytes at a stride of 64).  The live
// set is the two accumulators of the piece and FIT_AHEAD samples in flight, not the window.  m comes from one clock cell, so it is
// wave-uniform: the age loop has a scalar bound and the weights are uniform reads of the constant table.  The age loads are
// independent; FIT_AHEAD of them are issued before the first is used (ages past m - 1 are loaded where age m - 1 lies and not
// used).  Nothing is shared between threads: an instance's result depends neither on B nor on its neighbours.  No atomics, no LDS.
constexpr int FIT_AHEAD = 4;
__global__ __launch_bounds__(64) void k_scene_fit(int n_piece, int n_rows, int N, int window, SceneSrc seen, double* __restrict__ F) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_piece) return;
    const int rec_i = i / (SMPC_SCENE_ROW / 2), q = i % (SMPC_SCENE_ROW / 2);
    const int b = rec_i / n_rows, r = rec_i % n_rows;
    const int64_t t = scene_time(seen);
    const int64_t shown = (t < 0 ? 0 : t) + 1;
    const int m = shown < window ? (int)shown : window;
    const double* __restrict__ u = FIT_WEIGHTS.u + m * (m - 1) / 2;
    const double* __restrict__ w = FIT_WEIGHTS.w + m * (m - 1) / 2;
    const size_t piece = (size_t)r * SMPC_SCENE_ROW + 2 * q;
    const auto sample = [&](int j) {
        const int age = j < m ? j : m - 1;
        return *static_cast<const ScenePiece*>(__builtin_assume_aligned(scene_block(seen, b, t - age, n_rows) + piece, 16));
    };
    ScenePiece a{0.0, 0.0}, d{0.0, 0.0};
    for (int j0 = 0; j0 < m; j0 += FIT_AHEAD) {
        ScenePiece y[FIT_AHEAD];
#pragma unroll
        for (int e = 0; e < FIT_AHEAD; e++) y[e] = sample(j0 + e);
#pragma unroll
        for (int e = 0; e < FIT_AHEAD; e++) {
            const int j = j0 + e;
            if (j >= m) break;
            const ScenePiece pa{rounded_product(u[j], y[e].a), rounded_product(u[j], y[e].b)};
            const ScenePiece pd{rounded_product(w[j], y[e].a), rounded_product(w[j], y[e].b)};
            if (j == 0) {       // (a = u_0 y_0, not 0 + u_0 y_0: a -0.0 stays one)
                a = pa;
                d = pd;
            } else {
                a.a = a.a + pa.a; a.b = a.b + pa.b;
                d.a = d.a + pd.a; d.b = d.b + pd.b;
            }
        }
    }
    ScenePiece* out = static_cast<ScenePiece*>(__builtin_assume_aligned(F + (size_t)b * (size_t)(N + 1) * n_rows * SMPC_SCENE_ROW + piece, 16));
    const size_t step = (size_t)n_rows * (SMPC_SCENE_ROW / 2);      // in pieces
    *out = a;
    for (int k = 1; k <= N; k++) {
        a.a = a.a + d.a;
        a.b = a.b + d.b;
        out[k * step] = a;
    }
}

// The weights of a least-squares parabola y(tau) = a + b tau + c tau^2 through m equally spaced samples at tau = -j, ages j = 0..m-1,
// for m = 3..SMPC_FIT_MAX (rows 1 and 2 stay zero and are not read), and the weight of the window mean, 1 / m:
//   ua_j = (3(3m^2 - 3m + 2) - 18(2m - 1) j + 30 j^2)                        / (m (m + 1)(m + 2))      a, the value now
//   uv_j = ((36m^3 - 96m^2 + 36m + 24) + (-192m^2 + 180m + 48) j + 180 m j^2) / (m (m^2 - 1)(m^2 - 4))  v = b + c, the first step
//   ue_j = (60 ((m - 1)(m - 2) - 6(m - 1) j + 6 j^2))                        / (m (m^2 - 1)(m^2 - 4))  e = 2c, the step of the step
// Numerators stay below 2^31 and denominators reach 33 390 720 at m = 32, so the integers are formed in 64 bits; every weight is ONE
// correctly rounded division, done by the compiler: the bits of problem.poly_weights.  Row m starts at m (m - 1) / 2, as in
// FIT_WEIGHTS, and like it the table lies in the code object's constant data: no upload.
struct PolyWeights {
    double ua[SMPC_FIT_MAX * (SMPC_FIT_MAX + 1) / 2], uv[SMPC_FIT_MAX * (SMPC_FIT_MAX + 1) / 2], ue[SMPC_FIT_MAX * (SMPC_FIT_MAX + 1) / 2];
    double mean[SMPC_FIT_MAX + 1];
    constexpr PolyWeights() : ua{}, uv{}, ue{}, mean{} {
        for (long long m = 1; m <= SMPC_FIT_MAX; m++) {
            mean[m] = 1.0 / (double)m;
            if (m < 3) continue;
            const long long da = m * (m + 1) * (m + 2), dv = m * (m * m - 1) * (m * m - 4);
            for (long long j = 0; j < m; j++) {
                ua[m * (m - 1) / 2 + j] = (double)(3 * (3 * m * m - 3 * m + 2) - 18 * (2 * m - 1) * j + 30 * j * j) / (double)da;
                uv[m * (m - 1) / 2 + j] =
                    (double)((36 * m * m * m - 96 * m * m + 36 * m + 24) + (-192 * m * m + 180 * m + 48) * j + 180 * m * j * j) / (double)dv;
                ue[m * (m - 1) / 2 + j] = (double)(60 * ((m - 1) * (m - 2) - 6 * (m - 1) * j + 6 * j * j)) / (double)dv;
            }
        }
    }
};
__constant__ constexpr PolyWeights POLY_WEIGHTS{};

// k_scene_poly: F [B][N+1][n_rows][SMPC_SCENE_ROW] from S = seen.geom by a least-squares polynomial of degree 0 or 2 through the last
// `window` columns seen (degree 1 is k_scene_fit itself: the engine launches that).  With t, col, m and y_j as in k_scene_fit and the
// effective degree p = min(degree, m - 1) -- one sample gives a constant, two give a line -- for all eight slots
//   p = 0   a = u y_0;  a = a + u y_j,  u = 1 / m;                      F[b][k] = a, k = 0..N          -- stored, not added
//   p = 1   a and d of k_scene_fit with FIT_WEIGHTS (m = 2 only);       F[b][0] = a, F[b][k] = F[b][k-1] + d
//   p = 2   a, v, e each x = u_0 y_0;  x = x + u_j y_j  with ua, uv, ue;  F[b][0] = a,  F[b][k] = F[b][k-1] + v;  v = v + e
// every product rounded before its sum (rounded_product): problem.poly_forecast_statement operation for operation, so the kernel
// equals it bit for bit.  The mapping is k_scene_fit's and for its reasons: a thread owns ONE 16-byte piece of a record, four
// neighbouring lanes a whole 64-byte record, a wavefront's access 16 whole records; FIT_AHEAD age loads are issued before the first
// is used.  m and p come from one clock cell, so they are wave-uniform: the age loop has a scalar bound, the weights are uniform reads
// of the constant tables, and the branches on p are scalar -- the line's tail adds no zero e (-0.0 + 0.0 is not -0.0) and the
// constant's adds nothing.  The live set is three accumulators of the piece and FIT_AHEAD samples in flight.  Nothing is shared
// between threads: an instance's result depends neither on B nor on its neighbours.  No atomics, no LDS.
__global__ __launch_bounds__(64) void k_scene_poly(int n_piece, int n_rows, int N, int window, int degree, SceneSrc seen,
                                                   double* __restrict__ F) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_piece) return;
    const int rec_i = i / (SMPC_SCENE_ROW / 2), q = i % (SMPC_SCENE_ROW / 2);
    const int b = rec_i / n_rows, r = rec_i % n_rows;
    const int64_t t = scene_time(seen);
    const int64_t shown = (t < 0 ? 0 : t) + 1;
    const int m = shown < window ? (int)shown : window;
    const int p = degree < m - 1 ? degree : m - 1;
    const int row = m * (m - 1) / 2;
    const double* __restrict__ ua = p == 2 ? POLY_WEIGHTS.ua + row : FIT_WEIGHTS.u + row;
    const double* __restrict__ uv = p == 2 ? POLY_WEIGHTS.uv + row : FIT_WEIGHTS.w + row;
    const double* __restrict__ ue = POLY_WEIGHTS.ue + row;
    const double mean = POLY_WEIGHTS.mean[m];
    const size_t piece = (size_t)r * SMPC_SCENE_ROW + 2 * q;
    const auto sample = [&](int j) {
        const int age = j < m ? j : m - 1;
        return *static_cast<const ScenePiece*>(__builtin_assume_aligned(scene_block(seen, b, t - age, n_rows) + piece, 16));
    };
    ScenePiece a{0.0, 0.0}, v{0.0, 0.0}, e{0.0, 0.0};
    for (int j0 = 0; j0 < m; j0 += FIT_AHEAD) {
        ScenePiece y[FIT_AHEAD];
#pragma unroll
        for (int l = 0; l < FIT_AHEAD; l++) y[l] = sample(j0 + l);
#pragma unroll
        for (int l = 0; l < FIT_AHEAD; l++) {
            const int j = j0 + l;
            if (j >= m) break;
            const double wa = p == 0 ? mean : ua[j];
            const ScenePiece pa{rounded_product(wa, y[l].a), rounded_product(wa, y[l].b)};
            if (j == 0) {       // (x = u_0 y_0, not 0 + u_0 y_0: a -0.0 stays one)
                a = pa;
            } else {
                a.a = a.a + pa.a; a.b = a.b + pa.b;
            }
            if (p >= 1) {
                const ScenePiece pv{rounded_product(uv[j], y[l].a), rounded_product(uv[j], y[l].b)};
                if (j == 0) {
                    v = pv;
                } else {
                    v.a = v.a + pv.a; v.b = v.b + pv.b;
                }
            }
            if (p == 2) {
                const ScenePiece pe{rounded_product(ue[j], y[l].a), rounded_product(ue[j], y[l].b)};
                if (j == 0) {
                    e = pe;
                } else {
                    e.a = e.a + pe.a; e.b = e.b + pe.b;
                }
            }
        }
    }
    ScenePiece* out = static_cast<ScenePiece*>(__builtin_assume_aligned(F + (size_t)b * (size_t)(N + 1) * n_rows * SMPC_SCENE_ROW + piece, 16));
    const size_t step = (size_t)n_rows * (SMPC_SCENE_ROW / 2);      // in pieces
    *out = a;
    if (p == 2) {
        for (int k = 1; k <= N; k++) {
            a.a = a.a + v.a; a.b = a.b + v.b;
            v.a = v.a + e.a; v.b = v.b + e.b;
            out[k * step] = a;
        }
    } else if (p == 1) {
        for (int k = 1; k <= N; k++) {
            a.a = a.a + v.a; a.b = a.b + v.b;
            out[k * step] = a;
        }
    } else {
        for (int k = 1; k <= N; k++) out[k * step] = a;
    }
}

// k_fit_margin: the row-bounds table [lo | hi], each [B][N+1][n_rows], from the residuals of the fit that k_scene_fit / k_scene_poly
// forecast with -- the prediction interval of a least-squares polynomial per (instance, row, node); DESIGN.md section 9r.  With S, t,
// col, m, p and y_j as in k_scene_poly and a, v, e that kernel's numbers for every slot (the same operations in the same order):
//   nu = m - p - 1;   nu >= 1:  f_j = a | a - j v | (a - j v) + (j (j + 1) / 2) e   (p = 0 | 1 | 2),  res = y_j - f_j,
//                               q = res res at j = 0, q = q + res res afterwards;  rss = the largest q over the row kind's moving slots,
//                               a NaN winning;  s2 = rss / (double)nu, raised to var_prior where it is below it (a NaN stays)
//                     nu == 0:  s2 = var_prior
//   h_k = sum_j c_kj^2,  c_kj = 1 / m | u_j + k w_j | (ua_j + k uv_j) + (k (k - 1) / 2) ue_j,  in increasing j from the j = 0 term
//   d_k = (base_a + base_b k) + (z sqrt(s2)) sqrt(h_k);   d_k = d_k <= d_max ? d_k : d_max      -- a NaN gives the cap
// every product rounded before its sum (rounded_product): problem.fit_margin_statement operation for operation.  A row without a
// world-fixed element (SEG_SEG) has d = 0.  The bounds are problem.inflated_row_bounds': a plane row lb + d and ub - d, any other
// (sqrt(lb) + d)^2 with sqrt(lb) taken on the host, an absent side (|v| >= SMPC_INF) as it is, and the descriptor's own doubles where
// d == 0.0.
// One-wavefront blocks.  N + 1 <= 64, so lane k forms h_k and sqrt(h_k) once per block into N + 1 doubles of LDS: m and p come from
// one clock cell, so the age loop has a scalar bound and the weights are uniform reads of the constant tables.  Then k_scene_poly's
// mapping: four neighbouring lanes own the four 16-byte pieces of a record, FIT_AHEAD age loads in flight.  The first pass forms a, v,
// e; the second re-reads the window (m <= 32 columns of 64 bytes, hot in L2) for the residuals.  The maximum over the record's slots
// crosses its four lanes by two shuffles -- a maximum does not depend on order, so it keeps its bits -- and the four lanes then share
// the nodes for the stores.  No atomics; nothing is shared between instances, so an instance's result depends neither on B nor on its
// neighbours, and two calls give the same bits.
struct MarginRows {
    double lb[SMPC_MAX_ROWS], ub[SMPC_MAX_ROWS], sqrt_lb[SMPC_MAX_ROWS];
    int32_t kind[SMPC_MAX_ROWS];
};
struct MarginArgs { double z, var_prior, base_a, base_b, d_max; };
// a NaN wins: what np.maximum does
__device__ __forceinline__ double max_nan_wins(double best, double x) { return (x > best || x != x) ? x : best; }
__global__ __launch_bounds__(64) void k_fit_margin(int n_piece, int n_rows, int N, int window, int degree, SceneSrc seen, MarginArgs ma,
                                                   MarginRows rows, double* __restrict__ lo, double* __restrict__ hi) {
    __shared__ double g_lds[SMPC_MAX_N + 1];
    const int64_t t = scene_time(seen);
    const int64_t shown = (t < 0 ? 0 : t) + 1;
    const int m = shown < window ? (int)shown : window;
    const int p = degree < m - 1 ? degree : m - 1;
    const int nu = m - p - 1;
    const int row = m * (m - 1) / 2;
    const double* __restrict__ ua = p == 2 ? POLY_WEIGHTS.ua + row : FIT_WEIGHTS.u + row;
    const double* __restrict__ uv = p == 2 ? POLY_WEIGHTS.uv + row : FIT_WEIGHTS.w + row;
    const double* __restrict__ ue = POLY_WEIGHTS.ue + row;
    const double mean = POLY_WEIGHTS.mean[m];
    {   // the growth along the horizon: lane k forms g_k
        const int k = threadIdx.x;
        const double kd = (double)k, kk = (double)(k * (k - 1) / 2);
        double h = 0.0;
        for (int j = 0; j < m; j++) {
            double c = mean;
            if (p == 1) c = ua[j] + rounded_product(kd, uv[j]);
            if (p == 2) c = (ua[j] + rounded_product(kd, uv[j])) + rounded_product(kk, ue[j]);
            const double cc = rounded_product(c, c);
            h = j == 0 ? cc : h + cc;
        }
        if (k <= N) g_lds[k] = __builtin_sqrt(h);
    }
    __syncthreads();
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_piece) return;       // (n_piece is a multiple of four: the four lanes of a record leave together)
    const int rec_i = i / (SMPC_SCENE_ROW / 2), q = i % (SMPC_SCENE_ROW / 2);
    const int b = rec_i / n_rows, r = rec_i % n_rows;
    const int kind = rows.kind[r];
    // the record's moving slots (the ones set_scene_table validates) lie in [s_lo, s_hi); this lane holds slots 2q and 2q + 1
    const int s_lo = kind == SMPC_ROW_COORD ? 6 : 0;
    const int s_hi = kind == SMPC_ROW_SEG_FIXEDSEG ? 6 : (kind == SMPC_ROW_SEG_POINT || kind == SMPC_ROW_POINT_POINT ? 3 : (kind == SMPC_ROW_COORD ? 7 : 0));
    double s2 = ma.var_prior;
    if (nu >= 1 && s_hi > 0) {      // (scalar on nu; a record's four lanes agree on its kind)
        const size_t piece = (size_t)r * SMPC_SCENE_ROW + 2 * q;
        const auto sample = [&](int j) {
            const int age = j < m ? j : m - 1;
            return *static_cast<const ScenePiece*>(__builtin_assume_aligned(scene_block(seen, b, t - age, n_rows) + piece, 16));
        };
        ScenePiece a{0.0, 0.0}, v{0.0, 0.0}, e{0.0, 0.0};
        for (int j0 = 0; j0 < m; j0 += FIT_AHEAD) {
            ScenePiece y[FIT_AHEAD];
#pragma unroll
            for (int l = 0; l < FIT_AHEAD; l++) y[l] = sample(j0 + l);
#pragma unroll
            for (int l = 0; l < FIT_AHEAD; l++) {
                const int j = j0 + l;
                if (j >= m) break;
                const double wa = p == 0 ? mean : ua[j];
                const ScenePiece pa{rounded_product(wa, y[l].a), rounded_product(wa, y[l].b)};
                if (j == 0) {
                    a = pa;
                } else {
                    a.a = a.a + pa.a; a.b = a.b + pa.b;
                }
                if (p >= 1) {
                    const ScenePiece pv{rounded_product(uv[j], y[l].a), rounded_product(uv[j], y[l].b)};
                    if (j == 0) {
                        v = pv;
                    } else {
                        v.a = v.a + pv.a; v.b = v.b + pv.b;
                    }
                }
                if (p == 2) {
                    const ScenePiece pe{rounded_product(ue[j], y[l].a), rounded_product(ue[j], y[l].b)};
                    if (j == 0) {
                        e = pe;
                    } else {
                        e.a = e.a + pe.a; e.b = e.b + pe.b;
                    }
                }
            }
        }
        ScenePiece qq{0.0, 0.0};
        for (int j0 = 0; j0 < m; j0 += FIT_AHEAD) {
            ScenePiece y[FIT_AHEAD];
#pragma unroll
            for (int l = 0; l < FIT_AHEAD; l++) y[l] = sample(j0 + l);
#pragma unroll
            for (int l = 0; l < FIT_AHEAD; l++) {
                const int j = j0 + l;
                if (j >= m) break;
                ScenePiece f = a;
                if (p >= 1) {
                    const double jd = (double)j;
                    f.a = a.a - rounded_product(jd, v.a); f.b = a.b - rounded_product(jd, v.b);
                }
                if (p == 2) {
                    const double tj = (double)(j * (j + 1) / 2);
                    f.a = f.a + rounded_product(tj, e.a); f.b = f.b + rounded_product(tj, e.b);
                }
                const double ra = y[l].a - f.a, rb = y[l].b - f.b;
                const ScenePiece rr{rounded_product(ra, ra), rounded_product(rb, rb)};
                if (j == 0) {
                    qq = rr;
                } else {
                    qq.a = qq.a + rr.a; qq.b = qq.b + rr.b;
                }
            }
        }
        double rss = 0.0;
        if (2 * q >= s_lo && 2 * q < s_hi) rss = max_nan_wins(rss, qq.a);
        if (2 * q + 1 >= s_lo && 2 * q + 1 < s_hi) rss = max_nan_wins(rss, qq.b);
        rss = max_nan_wins(rss, __shfl_xor(rss, 1));
        rss = max_nan_wins(rss, __shfl_xor(rss, 2));
        const double var = rss / (double)nu;
        s2 = (var > ma.var_prior || var != var) ? var : ma.var_prior;
    }
    const double zs = rounded_product(ma.z, __builtin_sqrt(s2));
    const double lb = rows.lb[r], ub = rows.ub[r], root = rows.sqrt_lb[r];
    const bool has_lb = __builtin_fabs(lb) < SMPC_INF, has_ub = __builtin_fabs(ub) < SMPC_INF;
    const size_t at = (size_t)b * (size_t)(N + 1) * n_rows + r;
    for (int k = q; k <= N; k += SMPC_SCENE_ROW / 2) {
        double d = (ma.base_a + rounded_product(ma.base_b, (double)k)) + rounded_product(zs, g_lds[k]);
        d = d <= ma.d_max ? d : ma.d_max;
        if (s_hi == 0) d = 0.0;
        double l = lb, u = ub;
        if (d != 0.0) {
            if (kind == SMPC_ROW_COORD) {
                if (has_lb) l = lb + d;
                if (has_ub) u = ub - d;
            } else if (has_lb) {
                const double w = root + d;
                l = rounded_product(w, w);
            }
        }
        lo[at + (size_t)k * n_rows] = l;
        hi[at + (size_t)k * n_rows] = u;
    }
}

// k_forecast_context: the context rows of a scene-aware safe-set network from the same F, one thread per number:
//   ctx[b][k][i] = (float)((F[b][k][row_i][slot_i] - mean[i]) / std[i])       -- the expression of k_ctx_normalise
// sel: which (row, slot) of the scene context number i is, by value like nm (at most MLP_KPAD pairs: no device block to keep, and a
// captured launch carries its own).  A kernel of its own behind k_scene_forecast on the stream, so that the forecast kernel holds
// no division.
struct ForecastSel { int8_t row[MLP_KPAD], slot[MLP_KPAD]; };
__global__ __launch_bounds__(64) void k_forecast_context(long n, int n_ctx, int n_rows, const double* __restrict__ F, ForecastSel sel,
                                                         CtxNorm nm, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % n_ctx);
    const size_t bk = (size_t)(i / n_ctx);
    const double v = F[(bk * n_rows + sel.row[c]) * SMPC_SCENE_ROW + sel.slot[c]];
    out[i] = (float)((v - nm.mean[c]) / nm.std[c]);
}

// The obstacle filter: a Kalman filter per (instance, row) record over all eight slots with the record's gains.
// The model by value: the degree p (0: constant, 1: constant velocity, 2: constant acceleration), Q = q^2 G G' as the six numbers the
// host formed (problem.kalman_noise), r^2 and the prior variances.  Row kinds by value too: no device block to keep, and a captured
// launch carries its own.
struct KalmanArgs { int32_t degree, reserved; double q00, q01, q02, q11, q12, q22, r2, v02, a02, beta; };
struct KalmanKinds { int32_t kind[SMPC_MAX_ROWS]; };
struct KalmanCov { double p00, p01, p02, p11, p12, p22; };

// Phi P Phi' + Q with Phi = ((1, 1, 1/2), (0, 1, 1), (0, 0, 1)) cut to p + 1 components: problem.kalman_predict_cov operation for
// operation -- the rows of A = Phi P, then A Phi', then + Q; the entries of absent components pass through.  p is uniform.
__device__ __forceinline__ KalmanCov kalman_predict_cov(int p, const KalmanCov& P, const KalmanArgs& ka) {
    KalmanCov o = P;
    if (p == 0) {
        o.p00 = P.p00 + ka.q00;
    } else if (p == 1) {
        const double a00 = P.p00 + P.p01, a01 = P.p01 + P.p11;
        o.p00 = (a00 + a01) + ka.q00;
        o.p01 = a01 + ka.q01;
        o.p11 = P.p11 + ka.q11;
    } else {
        const double a00 = (P.p00 + P.p01) + rounded_product(0.5, P.p02);
        const double a01 = (P.p01 + P.p11) + rounded_product(0.5, P.p12);
        const double a02 = (P.p02 + P.p12) + rounded_product(0.5, P.p22);
        const double a11 = P.p11 + P.p12, a12 = P.p12 + P.p22;
        o.p00 = ((a00 + a01) + rounded_product(0.5, a02)) + ka.q00;
        o.p01 = (a01 + a02) + ka.q01;
        o.p02 = a02 + ka.q02;
        o.p11 = (a11 + a12) + ka.q11;
        o.p12 = a12 + ka.q12;
        o.p22 = P.p22 + ka.q22;
    }
    return o;
}

// the moving slots of a row kind lie in [lo, hi) (the ones set_scene_table validates); a robot-robot row has none
__device__ __forceinline__ int moving_lo(int kind) { return kind == SMPC_ROW_COORD ? 6 : 0; }
__device__ __forceinline__ int moving_hi(int kind) {
    return kind == SMPC_ROW_SEG_FIXEDSEG ? 6 : (kind == SMPC_ROW_SEG_POINT || kind == SMPC_ROW_POINT_POINT ? 3 : (kind == SMPC_ROW_COORD ? 7 : 0));
}

// k_scene_kalman<ADVANCE>: one step of the filter on state [B][n_rows][SMPC_KALMAN_REC] (ADVANCE: reading y = S[b][col(t)][r], t the
// scene clock's cell) and F [B][N+1][n_rows][SMPC_SCENE_ROW] from the state as it then is -- problem.kalman_statement operation for
// operation, so the kernel equals it bit for bit.  A record is pos[8] | vel[8] | acc[8] | P00 P01 P02 P11 P12 P22 | s2 | n: four
// 64-byte lines.  k_scene_poly's mapping and for its reasons: a thread owns ONE 16-byte piece of pos, vel and acc, four neighbouring
// lanes a whole record, a wavefront's access 16 whole records; one-wavefront blocks.  Each of the four lanes reads the record's last
// line and forms the six covariance numbers and the gains itself -- the same arithmetic on the same bits, cheaper than sending nine
// doubles across lanes -- and lane 0 of the four stores them.  What does cross the four lanes, by two __shfl_xor each: "observed" (an
// AND) and nis (a maximum), neither of which depends on order.  (n_piece is a multiple of four and a record's lanes agree on n and on
// "observed": they take every branch together.)  ONE division per record and step; every product rounded before its sum.  p is
// uniform, so the branches on it are scalar and the absent components cost no load, no store and no register.  Without ADVANCE no
// table is read and `seen` is not touched.  Nothing is shared between records: no atomics, no LDS, and an instance's result depends
// neither on B nor on its neighbours.
template <bool ADVANCE>
__global__ __launch_bounds__(64) void k_scene_kalman(int n_piece, int n_rows, int N, KalmanArgs ka, KalmanKinds kinds, SceneSrc seen,
                                                     double* __restrict__ state, double* __restrict__ F) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_piece) return;
    const int rec_i = i / (SMPC_SCENE_ROW / 2), q = i % (SMPC_SCENE_ROW / 2);
    const int b = rec_i / n_rows, r = rec_i % n_rows;
    const int p = ka.degree;
    ScenePiece* st = static_cast<ScenePiece*>(__builtin_assume_aligned(state + (size_t)rec_i * SMPC_KALMAN_REC, 16));   // 16 pieces
    const size_t piece = (size_t)r * SMPC_SCENE_ROW + 2 * q;
    ScenePiece pos = st[q], vel{0.0, 0.0}, acc{0.0, 0.0};
    if (p >= 1) vel = st[4 + q];
    if (p == 2) acc = st[8 + q];
    if constexpr (ADVANCE) {
        const ScenePiece t0 = st[12], t1 = st[13], t2 = st[14], t3 = st[15];
        const int64_t t = scene_time(seen);
        const ScenePiece y = *static_cast<const ScenePiece*>(__builtin_assume_aligned(scene_block(seen, b, t, n_rows) + piece, 16));
        const int kind = kinds.kind[r];
        const int s_lo = moving_lo(kind), s_hi = moving_hi(kind);
        const bool in_a = 2 * q >= s_lo && 2 * q < s_hi, in_b = 2 * q + 1 >= s_lo && 2 * q + 1 < s_hi;
        int obs = !((in_a && y.a != y.a) || (in_b && y.b != y.b));
        obs &= __shfl_xor(obs, 1);
        obs &= __shfl_xor(obs, 2);
        KalmanCov P{t0.a, t0.b, t1.a, t1.b, t2.a, t2.b};
        double s2 = t3.a, n = t3.b;
        bool changed = false, first = false;      // (first seen: the absent components are written too, as zero)
        if (n >= 1.0) {
            changed = true;
            if (p == 2) {
                pos.a = (pos.a + vel.a) + rounded_product(0.5, acc.a); pos.b = (pos.b + vel.b) + rounded_product(0.5, acc.b);
                vel.a = vel.a + acc.a; vel.b = vel.b + acc.b;
            } else if (p == 1) {
                pos.a = pos.a + vel.a; pos.b = pos.b + vel.b;
            }
            P = kalman_predict_cov(p, P, ka);
            if (obs) {
                const double inv = 1.0 / (P.p00 + ka.r2);
                const double k0 = rounded_product(P.p00, inv), k1 = rounded_product(P.p01, inv), k2 = rounded_product(P.p02, inv);
                const ScenePiece nu{y.a - pos.a, y.b - pos.b};
                pos.a = pos.a + rounded_product(k0, nu.a); pos.b = pos.b + rounded_product(k0, nu.b);
                if (p >= 1) { vel.a = vel.a + rounded_product(k1, nu.a); vel.b = vel.b + rounded_product(k1, nu.b); }
                if (p == 2) { acc.a = acc.a + rounded_product(k2, nu.a); acc.b = acc.b + rounded_product(k2, nu.b); }
                const KalmanCov M = P;
                P.p00 = M.p00 - rounded_product(k0, M.p00);
                if (p >= 1) {
                    P.p01 = M.p01 - rounded_product(k0, M.p01);
                    P.p11 = M.p11 - rounded_product(k1, M.p01);
                }
                if (p == 2) {
                    P.p02 = M.p02 - rounded_product(k0, M.p02);
                    P.p12 = M.p12 - rounded_product(k1, M.p02);
                    P.p22 = M.p22 - rounded_product(k2, M.p02);
                }
                double nis = 0.0;
                if (in_a) nis = max_nan_wins(nis, rounded_product(rounded_product(nu.a, nu.a), inv));
                if (in_b) nis = max_nan_wins(nis, rounded_product(rounded_product(nu.b, nu.b), inv));
                nis = max_nan_wins(nis, __shfl_xor(nis, 1));
                nis = max_nan_wins(nis, __shfl_xor(nis, 2));
                s2 = s2 + rounded_product(ka.beta, nis - s2);
                s2 = s2 < 1.0 ? 1.0 : s2;
                n = n + 1.0;
            }
        } else if (obs) {
            changed = first = true;
            pos = y;
            vel = ScenePiece{0.0, 0.0};
            acc = ScenePiece{0.0, 0.0};
            P = KalmanCov{ka.r2, 0.0, 0.0, p >= 1 ? ka.v02 : 0.0, 0.0, p == 2 ? ka.a02 : 0.0};
            s2 = 1.0;
            n = 1.0;
        }
        if (changed) {
            st[q] = pos;
            if (p >= 1 || first) st[4 + q] = vel;
            if (p == 2 || first) st[8 + q] = acc;
            if (q == 0) {
                st[12] = ScenePiece{P.p00, P.p01};
                st[13] = ScenePiece{P.p02, P.p11};
                st[14] = ScenePiece{P.p12, P.p22};
                st[15] = ScenePiece{s2, n};
            }
        }
    }
    ScenePiece* out = static_cast<ScenePiece*>(__builtin_assume_aligned(F + (size_t)b * (size_t)(N + 1) * n_rows * SMPC_SCENE_ROW + piece, 16));
    const size_t step = (size_t)n_rows * (SMPC_SCENE_ROW / 2);      // in pieces
    *out = pos;
    if (p == 2) {
        ScenePiece v{vel.a + rounded_product(0.5, acc.a), vel.b + rounded_product(0.5, acc.b)};
        for (int k = 1; k <= N; k++) {
            pos.a = pos.a + v.a; pos.b = pos.b + v.b;
            v.a = v.a + acc.a; v.b = v.b + acc.b;
            out[k * step] = pos;
        }
    } else if (p == 1) {
        for (int k = 1; k <= N; k++) {
            pos.a = pos.a + vel.a; pos.b = pos.b + vel.b;
            out[k * step] = pos;
        }
    } else {
        for (int k = 1; k <= N; k++) out[k * step] = pos;
    }
}

// k_kalman_margin: the row-bounds table [lo | hi], each [B][N+1][n_rows], from the filter's own covariance -- problem.
// kalman_margin_statement operation for operation.  It reads P and s2 of a record (its last 64-byte line) and nothing else: no table,
// no clock.  Pi_0 = P, Pi_k = kalman_predict_cov(Pi_{k-1}), g_k = sqrt(Pi_k[0][0]); d_k = (base_a + base_b k) + (z sqrt(s2)) g_k,
// d_k = d_k <= d_max ? d_k : d_max (a NaN gives the cap); d = 0 for a row without a moving slot; the bounds are k_fit_margin's, the
// descriptor's own doubles where d == 0.0.  The walk along the horizon is a recurrence, so a thread owns a record and its N + 1 nodes:
// at node k neighbouring threads store neighbouring rows.  One-wavefront blocks; no atomics, no LDS, nothing shared between records.
__global__ __launch_bounds__(64) void k_kalman_margin(int n_rec, int n_rows, int N, KalmanArgs ka, MarginArgs ma, MarginRows rows,
                                                      const double* __restrict__ state, double* __restrict__ lo, double* __restrict__ hi) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n_rec) return;
    const int b = i / n_rows, r = i % n_rows;
    const int p = ka.degree;
    const int kind = rows.kind[r];
    const int s_hi = moving_hi(kind);
    const ScenePiece* st = static_cast<const ScenePiece*>(__builtin_assume_aligned(state + (size_t)i * SMPC_KALMAN_REC, 16));
    const ScenePiece t0 = st[12], t1 = st[13], t2 = st[14], t3 = st[15];
    KalmanCov Pi{t0.a, t0.b, t1.a, t1.b, t2.a, t2.b};
    const double zs = rounded_product(ma.z, __builtin_sqrt(t3.a));
    const double lb = rows.lb[r], ub = rows.ub[r], root = rows.sqrt_lb[r];
    const bool has_lb = __builtin_fabs(lb) < SMPC_INF, has_ub = __builtin_fabs(ub) < SMPC_INF;
    const size_t at = (size_t)b * (size_t)(N + 1) * n_rows + r;
    for (int k = 0; k <= N; k++) {
        double d = (ma.base_a + rounded_product(ma.base_b, (double)k)) + rounded_product(zs, __builtin_sqrt(Pi.p00));
        d = d <= ma.d_max ? d : ma.d_max;
        if (s_hi == 0) d = 0.0;
        double l = lb, u = ub;
        if (d != 0.0) {
            if (kind == SMPC_ROW_COORD) {
                if (has_lb) l = lb + d;
                if (has_ub) u = ub - d;
            } else if (has_lb) {
                const double w = root + d;
                l = rounded_product(w, w);
            }
        }
        lo[at + (size_t)k * n_rows] = l;
        hi[at + (size_t)k * n_rows] = u;
        Pi = kalman_predict_cov(p, Pi, ka);
    }
}

}  // namespace smpc
