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

}  // namespace smpc
