// engine.hip -- C ABI (include/smpc.h) of the MI355X batched safe-MPC engine: handle, device buffers, kernel launches.
// Built for gfx950 only:  hipcc --offload-arch=gfx950 -O3 -shared -fPIC engine.hip -o libsmpc_hip.so
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/smpc.h"
#include "kernel_qp.hpp"
#include "kernel_qp_wg.hpp"
#include "kernel_build.hpp"
#include "kernels_callers.hpp"
#include "kernels_policy.hpp"
#include "kernels_mlp.hpp"
#include "kernels_nodes.hpp"
#include "kernels_sqp.hpp"
#include "kernels_guess.hpp"
#include "kernels_score.hpp"
#include "kernels_ik.hpp"
#include "kernels_rays.hpp"
#include "kernels_forecast.hpp"

using namespace smpc;

namespace {
thread_local char g_create_err[256] = "";
}

// A device buffer owned by a handle: grown on demand, never shrunk, freed with the handle.  reserve() (below the handle) is the
// engine's one place that synchronises the stream, frees and allocates for growth.
template <class T> struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;     // bytes
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int reserve(smpc_handle* h, const char* what, size_t bytes, bool zero = false);
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// A small block of host arrays on the device, with the host's copy of what it holds: uploaded only when the image changes, so an
// unchanged call neither synchronises nor copies (upload(), below the handle).
struct ParamBlock {
    const char* what;       // the block's name in messages
    DevBuf<double> d;
    std::vector<double> cache;
    int upload(smpc_handle* h, std::vector<double>& img);
};

// A device array per instance: valid for exactly the batch size it was set with.  A setter makes room, fills
// the buffer (upload(), or work of its own on the handle's stream) and commits; readers take for_batch(B).  The members are defined
// below the handle.
struct SlotTag {
    const char *noun, *setter;      // in messages: "instance scene", "smpc_set_instance_scene"
    int B = 0;                      // the batch size the content is valid for; 0: none
    void clear() { B = 0; }
    void commit(int b) { B = b; }
    // an entry point that reads the slot refuses any other B while it is set, never the shared input instead without a word
    int guard(smpc_handle* h, int b, const char* who) const;
};
template <class T> struct InstSlot : SlotTag {
    DevBuf<T> d;
    InstSlot(const char* noun_, const char* setter_) : SlotTag{noun_, setter_} {}
    const T* held() const { return B ? d.p : nullptr; }                       // for a reader whose entry point has guarded its B
    const T* for_batch(int b) const { return B == b ? held() : nullptr; }     // for one that falls back to the shared input
    // Room for n elements, grown only when n grows: the same size is overwritten in place, stream-ordered, and a captured step keeps
    // seeing this buffer.  A failed growth leaves the slot empty; a refused one (capture) keeps the old content in force.
    int room(smpc_handle* h, size_t n, bool zero = false);
    // stream-ordered copy of n elements; a host source may be reused by the caller on return, so the stream is drained for it
    int upload(smpc_handle* h, const T* src, size_t n, bool on_device, size_t at = 0);
};

// What smpc_set_mlp, smpc_set_mlp_activation and smpc_set_mlp_context establish.  A handle owns one and reads the network through
// smpc_handle::net, which names its parent's in a worker of smpc_rollout_batch.
struct Net {
    int nlayers = 0;
    int act = SMPC_ACT_GELU_TANH;
    int dims[SMPC_MAX_LAYERS + 1] = {0};
    int H = 0;
    DevBuf<char> d_weights;         // one block for the three arrays below, 256-byte aligned
    float* Wfwd[SMPC_MAX_LAYERS] = {nullptr};  // [K][N] = W^T (layer 0 padded to MLP_KPAD rows)
    float* Wbwd[SMPC_MAX_LAYERS] = {nullptr};  // [out][in] as given (layer 0 padded to MLP_NPAD columns)
    float* bias[SMPC_MAX_LAYERS] = {nullptr};
    // the network's context (smpc_set_mlp_context): n_ctx numbers of the instance's scene behind the 2 nn_dof
    // state features of layer 0's input
    int n_ctx = 0;                  // 0: a network without context columns
    double ctx_mean[MLP_KPAD] = {0}, ctx_std[MLP_KPAD] = {0};
    DevBuf<float> d_default_ctx;    // [MLP_KPAD] the normalised default context
};

struct smpc_handle {
    smpc_problem_desc desc;
    int device = 0;
    int N = 0;
    hipStream_t stream = nullptr;
    smpc_problem_desc* d_desc = nullptr;
    DevBuf<double> d_lo, d_hi;      // [N+1][nx] stage bounds
    DevBuf<double> d_zl;            // [N+1] run-time slack weights of the soft safe-set rows (cost_set); empty: the formulation's
    // the per-instance inputs (InstSlot).  Unset: every launcher takes the shared input -- the descriptor's scene, the caller's
    // reference table (or none), the default context row, the shared stage bounds.
    InstSlot<double> bounds{"per-instance bounds", "smpc_set_instance_bounds"};     // [lo | hi], a half of the buffer each, both
                                                                                    // [B][N+1][nx] (RealReceding); not guarded
    InstSlot<double> scene{"instance scene", "smpc_set_instance_scene"};    // [B][T][n_rows][SMPC_SCENE_ROW] obstacle geometry along
                                                                            // time (smpc_set_instance_scene_track; _scene: T = 1)
    int64_t scene_T = 1;            // time columns of the scene
    const int64_t* scene_clock = nullptr;   // the caller's device cell of smpc_set_scene_clock; null: time 0
    bool scene_fc = false;          // the scene holds a forecast (smpc_forecast_scene): N + 1 columns read from time 0, no clock.
                                    // Assigned with every commit of the slot, so it means something only while the slot is set
    InstSlot<double> world{"instance world track", "smpc_set_instance_world_track"};    // [B][T][n_rows][SMPC_SCENE_ROW] the track the
                                    // plant meets: read by smpc_forecast_scene and smpc_loop_post alone
    int64_t world_T = 1;
    InstSlot<double> seen{"instance observed track", "smpc_set_instance_observed_track"};   // the world's layout: what the controller
                                    // observes of it.  While set, smpc_forecast_scene (HOLD, CV) and
                                    // smpc_forecast_scene_fit / _poly read it instead of the world; nothing else reads it
    int64_t seen_T = 1;
    InstSlot<double> curves{"instance curve table", "smpc_set_instance_curves"};    // [B][3][L] reference curves
    int64_t curves_L = 0;
    InstSlot<float> ctx{"instance context", "smpc_set_instance_context"};   // [B][T][n_ctx] normalised context of the network along
                                                                            // time (smpc_set_instance_context_track; _context: T = 1)
    int64_t ctx_T = 1;              // time columns of the context
    bool ctx_fc = false;            // the context was written by smpc_forecast_scene: read from time 0 (as scene_fc)
    InstSlot<smpc_joint> models{"instance model table", "smpc_set_instance_models"};    // [B][nq] the controller's joint records:
                                                                                        // the caller's inertials, the descriptor's rest
    InstSlot<double> rowb{"instance row-bounds table", "smpc_set_instance_row_bounds"};   // [lo | hi], each [B][N+1][n_rows]: the
                                    // collision rows' bounds per instance and node, read from node 0 without a
                                    // clock by the stage builders and k_merit alone; laid out by the horizon, like `bounds`
    // network
    Net own_net;
    const Net* net = &own_net;      // the network this handle runs: its own, or the parent's in a worker of smpc_rollout_batch
    // per-batch scratch of the solve path (ensure_batch)
    DevBuf<double> d_ev;    // linearisation records of the last call, interleaved tiles of EV_TILE nodes (device_model.hpp)
    DevBuf<double> d_nn;    // value and gradient of the network's row (read by the stage builder): [B][N+1][1 + nx] with the row
                            // on every node, [B][1 + nx] with the row on the end node only, empty without a network row; zeroed
                            // when allocated
    DevBuf<double> d_ws;
    int qp_mode = -2;       // smpc_set_qp_mode: SMPC_QP_AUTO / _THROUGHPUT / _LATENCY; -2 = not set (the process default, SMPC_QP_WG)
    DevBuf<double> d_hrec;  // k_qp_ipm_wg only: the stages' P-independent blocks, [B][N+1][HRecLayout::SIZE] (grown for a batch that
                            // takes the latency form only)
    bool wg_lds_raised[2] = {false, false};   // dynamic-LDS limit raised for this handle's instantiation of k_qp_ipm_wg (8 / 4 half-waves)
    DevBuf<int32_t> d_order, d_last_it;       // longest-first dispatch order from the previous call's iterations
    int order_B = 0;                          // batch size d_last_it is valid for (0 = none yet)
    DevBuf<int32_t> d_ord_hist;   // [256] histogram of d_last_it (k_qp_ipm) | [256] bin cursors | ticket (k_order_by_iters) | pair
                                  // ticket (k_qp_ipm's crew); zeroed when allocated
    double qp_crew = -1.0;        // smpc_set_qp_crew: wavefronts of a k_qp_ipm launch as a fraction of its pairs; < 0 = not set (the
    int qp_crew_waves = 0;        // process default, SMPC_QP_CREW) | > 0: that many wavefronts whatever the batch
    // MLP activations (ensure_mlp)
    DevBuf<float> d_S, d_y, d_GS, d_dA, d_dB;
    DevBuf<int32_t> d_nn_idx;     // compacted list of the nodes whose safe-set row is on, followed by its length d_nn_cnt
    int32_t* d_nn_cnt = nullptr;
                                // INVARIANT: *d_nn_cnt is zero whenever no chain of kernels is using it.  Every chain that fills it ends in
                                // something that hands it back at zero -- on the solve path a kernel that runs anyway (k_stage_build after the
                                // network pass, k_policy_post after the safe-set test), elsewhere a memset -- so the hot path has no memset
                                // launch of its own, and a captured step can be replayed whatever ran in between
    DevBuf<float> d_act[SMPC_MAX_LAYERS];
    DevBuf<float> d_dg[SMPC_MAX_LAYERS];
    DevBuf<char> d_stage;       // staging of the host-pointer calls (Stage)
    // The small host arrays of four entry points, each in a block of its own: the policy entry points keep chk warm with their own
    // values, and a shared block would make alternating callers upload on every call.
    ParamBlock chk{"check bounds"};                    // smpc_check_trajectory, smpc_policy_step, smpc_loop_post (chk_block)
    ParamBlock gchk{"guess check bounds"};             // smpc_check_guess (gchk_block)
    ParamBlock schk{"score bounds"};                   // smpc_score_rollout (schk_block)
    ParamBlock ikb{"inverse kinematics bounds"};       // smpc_ik_batch (ikb_block)
    DevBuf<char> d_roll;        // smpc_rollout_batch's scratch of the sub-batch this handle steps (RollScratch)
    // timing
    int timing = 0;
    int timed = 0;              // a solve has been timed since timing was enabled
    // a ring of timing-event sets, one per solve: a loop that enqueues far ahead of the GPU reads the per-kernel times of its
    // last EV_RING solves afterwards (smpc_get_timing_history), without a synchronisation inside the loop
    static constexpr int EV_RING = 64;
    hipEvent_t ev_sets[EV_RING][5] = {};
    bool ev_complete[EV_RING] = {};   // all five events of the slot were recorded by ONE solve (cleared when the slot is reused)
    hipEvent_t* ev_t = ev_sets[0];
    int ev_cur = 0;
    bool timing_now = false;    // this solve records its events (timing on and the stream is not being captured into a graph)
    long timed_count = 0;       // solves timed since timing was enabled
    // sub-batch workers of smpc_rollout_batch: full handles on their own streams that borrow this handle's network weights
    std::vector<smpc_handle*> kids;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    DevBuf<unsigned long long> d_wstat;   // [4] load-balance probe of k_qp_ipm (timing mode 1)
    const uint8_t* d_active = nullptr;   // smpc_policy_step only: instances the QP kernels skip (borrowed for the call)
    DevBuf<char> d_polw;        // scratch of the policy entry points (PolScratch)
    float last_ms[4] = {0, 0, 0, 0};
    long mlp_rows_whole = 0;    // > 0 (a worker of smpc_rollout_batch): network rows of the WHOLE call, which selects the network kernel
    long mlp_rows_hint = 0;     // > 0 (smpc_policy_step of the receding policies): the rows EXPECTED to be live in a compacted list -- one or
                                // two nodes per instance, where the list's capacity is every node -- which selects the network kernel
                                // (the count itself is only known on the device; any kernel is correct for any count)
    DevBuf<char> d_par;         // SMPC_POLICY_PARALLEL's candidate buffers (ParScratch), zeroed when allocated
    DevBuf<char> d_sqp;         // scratch of smpc_sqp_batch / smpc_merit_terms (SqpScratch)
    DevBuf<int32_t> d_guess;    // scratch of smpc_check_guess: pos[B], where an instance's safe-set row sits in the network pass's list
    DevBuf<char> d_score;       // scratch of smpc_score_rollout (ScoreScratch): the segments' partials and the running safe-set minimum
    char err[256] = "";
};

namespace {

int fail(smpc_handle* h, int code, const char* fmt, ...) {
    char* dst = h ? h->err : g_create_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 256, fmt, ap);
    va_end(ap);
    return code;
}
#define HIPCHK(h, expr)                                                                                       \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return fail(h, SMPC_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));        \
    } while (0)

// the handle's stream is being captured into a hipGraph (directly or by joining a capture through an event)
bool capturing(const smpc_handle* h) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(h->stream, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}

}  // namespace

// Growth is refused while the stream is being captured: synchronising it would invalidate the capture.  A failed allocation
// leaves the buffer empty.
template <class T> int DevBuf<T>::reserve(smpc_handle* h, const char* what, size_t bytes, bool zero) {
    if (bytes <= cap) return SMPC_OK;
    if (capturing(h))
        return fail(h, SMPC_ESTATE, "the %s must grow from %zu to %zu bytes while the stream is being captured: run one eager call "
                    "of this size first", what, cap, bytes);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    release();
    const hipError_t e = hipMalloc((void**)&p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        return fail(h, SMPC_ENOMEM, "hipMalloc(%zu bytes) for the %s failed: %s", bytes, what, hipGetErrorString(e));
    }
    if (zero) HIPCHK(h, hipMemsetAsync(p, 0, bytes, h->stream));
    cap = bytes;
    return SMPC_OK;
}

// The one upload of a parameter block.  A copy from pageable host memory waits for the stream to drain, which would turn every
// per-step call of a device-resident loop into a host synchronisation: hence only on change.  A change is refused while the stream
// is being captured, like growth: synchronising would invalidate the capture.  img is left holding the previous image.
int ParamBlock::upload(smpc_handle* h, std::vector<double>& img) {
    int rc;
    if ((rc = d.reserve(h, what, img.size() * sizeof(double)))) return rc;
    if (img == cache) return SMPC_OK;
    if (capturing(h))
        return fail(h, SMPC_ESTATE, "the %s changed while the stream is being captured: run one eager call with these bounds first", what);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(d.p, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice));
    cache.swap(img);
    return SMPC_OK;
}

int SlotTag::guard(smpc_handle* h, int b, const char* who) const {
    if (B && B != b)
        return fail(h, SMPC_EINVAL, "%s: batch size %d, but the %s was set for %d instances (%s: clear it or set one of this size)", who, b,
                    noun, B, setter);
    return SMPC_OK;
}
template <class T> int InstSlot<T>::room(smpc_handle* h, size_t n, bool zero) {
    const int rc = d.reserve(h, noun, n * sizeof(T), zero);
    if (rc && !d.p) clear();
    return rc;
}
template <class T> int InstSlot<T>::upload(smpc_handle* h, const T* src, size_t n, bool on_device, size_t at) {
    HIPCHK(h, hipMemcpyAsync(d.p + at, src, n * sizeof(T), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    if (!on_device) HIPCHK(h, hipStreamSynchronize(h->stream));
    return SMPC_OK;
}

namespace {

// An entry point that cannot honour per-instance inputs at all refuses each of the given slots while it is set.
int refuse_slots(smpc_handle* h, const char* who, const char* why, std::initializer_list<const SlotTag*> slots) {
    for (const SlotTag* s : slots)
        if (s->B)
            return fail(h, SMPC_ESTATE, "%s: an %s is set (for %d instances) and %s: clear it (%s with a NULL array)", who, s->noun, s->B,
                        why, s->setter);
    return SMPC_OK;
}

// Bump allocator, 256-byte alignment unless told otherwise: with a null base it only sizes a layout (off), with a buffer's base it
// places it.
struct Carve {
    char* base;
    size_t off = 0;
    size_t align = 256;
    template <class T> T* take(size_t n) {
        T* q = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (sizeof(T) * n + align - 1) & ~(align - 1);
        return q;
    }
};

// A parameter block's arrays follow one another without padding (what the kernels were given before the blocks had layouts): the
// *_block functions below state each block once, on the host image for the fill and on the device block for the launcher.
Carve dense(double* base) { return Carve{reinterpret_cast<char*>(base), 0, sizeof(double)}; }
void put(double* dst, const double* src, int n) {
    if (n > 0) memcpy(dst, src, sizeof(double) * n);
}

// f(std::integral_constant<int, NQ>{}) with the handle's joint count as the kernels' compile-time constant
template <class F> int with_nq(smpc_handle* h, F&& f) {
    switch (h->desc.nq) {
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return fail(h, SMPC_EINVAL, "nq=%d not built (5, 6, 7)", h->desc.nq);
    }
}

// Device views of an entry point's array arguments.  Host pointers (on_device == 0): in() uploads an input into the handle's
// staging buffer, out() is a staged array that finish() copies back (a null host pointer: scratch only), inout() both, and
// finish() waits for the copies.  place() runs the caller's `views` twice, to size the staging buffer (null base) and then on
// it.  Device pointers: every view is the caller's own pointer, the staging buffer is not touched and finish() does nothing.
struct Stage {
    smpc_handle* h;
    bool dev;
    Carve c{nullptr};
    hipError_t e = hipSuccess;
    struct Back {
        void* host;
        const void* dev;
        size_t bytes;
    };
    std::vector<Back> back;

    template <class T> T* view(T* host, size_t n, bool up, bool down) {
        if (dev || (up && !host)) return host;       // (a null input is an absent optional one)
        auto* d = c.take<std::remove_const_t<T>>(n);
        if (!d) return nullptr;                       // (sizing pass)
        if (up && e == hipSuccess) e = hipMemcpyAsync(d, host, sizeof(T) * n, hipMemcpyHostToDevice, h->stream);
        if (down && host) back.push_back({(void*)host, d, sizeof(T) * n});
        return d;
    }
    template <class T> const T* in(const T* host, size_t n) { return view(host, n, true, false); }
    template <class T> T* out(T* host, size_t n) { return view(host, n, false, true); }
    template <class T> T* inout(T* host, size_t n) { return view(host, n, true, true); }

    template <class F> int place(F&& views) {
        views(*this);
        if (dev) return SMPC_OK;
        int rc;
        if ((rc = h->d_stage.reserve(h, "staging buffer", c.off))) return rc;
        c = Carve{h->d_stage.p};
        views(*this);
        if (e != hipSuccess) return fail(h, SMPC_EHIP, "staging copy failed: %s", hipGetErrorString(e));
        return SMPC_OK;
    }
    int finish() {
        if (dev) return SMPC_OK;
        for (const Back& b : back) HIPCHK(h, hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return SMPC_OK;
    }
};

size_t ws_doubles_per_instance(smpc_handle* h, int N) {
    size_t per = 0;     // (smpc_create admits no handle with another nq)
    with_nq(h, [&](auto NQ) { per = QpLayout<NQ>(h->desc.n_rows).per_instance(N); return SMPC_OK; });
    return per;
}

int upload_bounds(smpc_handle* h, const double* lo, const double* hi) {
    const int nx = 2 * h->desc.nq;
    std::vector<double> l((size_t)(h->N + 1) * nx), u((size_t)(h->N + 1) * nx);
    for (int k = 0; k <= h->N; k++)
        for (int i = 0; i < nx; i++) {
            l[(size_t)k * nx + i] = lo ? lo[(size_t)k * nx + i] : (k == h->N ? h->desc.x_lo_e[i] : h->desc.x_lo[i]);
            u[(size_t)k * nx + i] = hi ? hi[(size_t)k * nx + i] : (k == h->N ? h->desc.x_hi_e[i] : h->desc.x_hi[i]);
        }
    int rc;
    if ((rc = h->d_lo.reserve(h, "stage bounds", l.size() * sizeof(double))) ||
        (rc = h->d_hi.reserve(h, "stage bounds", u.size() * sizeof(double))))
        return rc;
    HIPCHK(h, hipMemcpyAsync(h->d_lo.p, l.data(), l.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_hi.p, u.data(), u.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SMPC_OK;
}

// the network pass's buffers for M rows: level 0 the output alone (k_mlp_fused), 1 also the hidden layers' activation derivatives
// (k_mlp_wave), 2 every buffer of the layer-by-layer GEMM chain
int ensure_mlp(smpc_handle* h, size_t M, int level = 2) {
    const size_t Mp = (M + 127) / 128 * 128, row = sizeof(float) * Mp, H = h->net->H;
    int rc;
    if ((rc = h->d_y.reserve(h, "network output", row))) return rc;
    for (int l = 0; level >= 1 && l + 1 < h->net->nlayers; l++)
        if ((rc = h->d_dg[l].reserve(h, "network activation derivatives", row * H))) return rc;
    if (level < 2) return SMPC_OK;
    if ((rc = h->d_S.reserve(h, "network features", row * MLP_KPAD)) || (rc = h->d_GS.reserve(h, "network gradients", row * MLP_NPAD)) ||
        (rc = h->d_dA.reserve(h, "network backward pass", row * H)) || (rc = h->d_dB.reserve(h, "network backward pass", row * H)))
        return rc;
    for (int l = 0; l + 1 < h->net->nlayers; l++)
        if ((rc = h->d_act[l].reserve(h, "network activations", row * H))) return rc;
    return SMPC_OK;
}

// list of live network rows (mode 3 of run_mlp) and its device-side length d_nn_cnt, the buffer's last entry, zeroed when allocated
int ensure_nn_idx(smpc_handle* h, size_t M) {
    if (sizeof(int32_t) * (M + 1) <= h->d_nn_idx.cap) return SMPC_OK;
    const int rc = h->d_nn_idx.reserve(h, "network row list", sizeof(int32_t) * (M + 1));
    // (the counter follows the buffer whatever the outcome: a refused growth keeps the old list and its counter, a failed one
    //  leaves neither)
    h->d_nn_cnt = h->d_nn_idx.cap ? h->d_nn_idx.p + h->d_nn_idx.cap / sizeof(int32_t) - 1 : nullptr;
    if (rc) return rc;
    HIPCHK(h, hipMemsetAsync(h->d_nn_cnt, 0, sizeof(int32_t), h->stream));
    return SMPC_OK;
}

// Which instance a network row belongs to (CtxSrc, kernels_mlp.hpp): node / per on instance-major node arrays with `per` nodes per
// instance, the node of its instance being the node-time index of a context track; (m0 + m) % B on a step-major log read from flat
// row m0, whose state index (m0 + m) / B counts time from 0 (run_mlp hands the kernels no clock cell there).
CtxSrc rows_of_nodes(int per) { CtxSrc c; c.per = per; return c; }
CtxSrc rows_step_major(int B, long m0) { CtxSrc c; c.mod = B; c.m0 = (int)(m0 % B); c.j0 = (int)(m0 / B); return c; }

// forward (and optionally backward) pass of the network over M rows whose states are found through (mode, N) in x.
// mode 3: the rows are the compacted list h->d_nn_idx of live nodes; their count is only known on the device (h->d_nn_cnt), so
// the grids cover all M candidate rows and the blocks past the count return at once.
// d_p / d_ev: when given and the pass ran as the fused kernel, the chain rule to the node records is done as well and *chained
// is set (the caller then skips k_nn_chain).
// rows: which instance a row belongs to (rows_of_nodes / rows_step_major), for the context of a network that has one; the table it
// indexes is the handle's.
template <int NQ> int run_mlp(smpc_handle* h, int M, int mode, int N, const double* d_x, bool backward, CtxSrc rows,
                              const double* d_p = nullptr, double* d_ev = nullptr, bool* chained = nullptr, int compact = 0) {
    int rc;
    // the instances' own rows when they are set (every entry point has checked its B against the slot's: guard), else the default row
    // for all; without context columns the kernels' context loop has no iteration
    const Net& net = *h->net;
    CtxSrc cx = rows;
    if (net.n_ctx > 0) {
        const float* own = h->ctx.held();
        cx.n = net.n_ctx;
        cx.p = own ? own : net.d_default_ctx.p;
        cx.stride = own ? net.n_ctx : 0;
        // a track: the column of a row follows the scene clock on the node arrays, the state index alone on the log (rows_step_major);
        // a single column needs no time, so the clock is not handed on with T = 1 (as with_scene)
        cx.T = own ? (int)h->ctx_T : 1;
        cx.clock = cx.T > 1 && cx.mod == 0 && !(own && h->ctx_fc) ? h->scene_clock : nullptr;     // (a forecast: from time 0)
    }
    const int Mp = (M + 127) / 128 * 128, H = net.H, L = net.nlayers;
    hipStream_t s = h->stream;
    const int32_t* idx = mode == 3 ? h->d_nn_idx.p : nullptr;
    const int32_t* live = mode == 3 ? h->d_nn_cnt : nullptr;
    if (chained) *chained = false;
    // Few rows (the terminal row: M = B): the whole pass as ONE kernel, activations in LDS / registers (kernels_mlp.hpp).  The
    // choice follows the rows of the whole call (mlp_rows_whole).
    {
        const long rows_all = h->mlp_rows_whole > 0 ? (h->mlp_rows_whole + 127) / 128 * 128
                                                    : (h->mlp_rows_hint > 0 && mode == 3 ? (h->mlp_rows_hint + 127) / 128 * 128 : (long)Mp);
        static const bool no_fused = getenv("SMPC_MLP_UNFUSED") != nullptr;     // (A/B knob)
        static const long fused_max = [] { const char* e = getenv("SMPC_MLP_FUSED_MAX"); return e ? atol(e) : 8192L; }();   // (A/B knob)
        if (!no_fused && rows_all < fused_max && H == MLPF_H && L == 4 && (!backward || (d_p && d_ev))) {
            if ((rc = ensure_mlp(h, (size_t)M, 0))) return rc;
            MlpWeights Wt;
            for (int l = 0; l < SMPC_MAX_LAYERS; l++) { Wt.wf[l] = net.Wfwd[l]; Wt.wb[l] = net.Wbwd[l]; Wt.bias[l] = net.bias[l]; }
            const dim3 grd((M + MLPF_ROWS - 1) / MLPF_ROWS), blk(256);
            if (backward)
                hipLaunchKernelGGL((k_mlp_fused<NQ, true>), grd, blk, 0, s, h->d_desc, M, N, mode, net.act, Wt, d_x, d_p, idx, live, h->d_y.p, d_ev,
                                   compact, cx);
            else
                hipLaunchKernelGGL((k_mlp_fused<NQ, false>), grd, blk, 0, s, h->d_desc, M, N, mode, net.act, Wt, d_x, d_p, idx, live, h->d_y.p,
                                   (double*)nullptr, 0, cx);
            HIPCHK(h, hipGetLastError());
            if (chained) *chained = backward;
            return SMPC_OK;
        }
        // Many rows (the row on every node): the same pass as ONE-WAVE blocks (k_mlp_wave, round 5) -- a block fits where a single QP
        // wavefront has retired, and only the activation derivatives leave the chip.  SMPC_MLP_LARGE=chain brings the layer-by-layer
        // GEMMs back (A/B runs; they also serve any network that is not 256 wide with three hidden layers).
        static const bool large_chain = [] { const char* e = getenv("SMPC_MLP_LARGE"); return e && !strcmp(e, "chain"); }();
        if (!no_fused && !large_chain && rows_all >= fused_max && H == MLPF_H && L == 4 && (!backward || (d_p && d_ev))) {
            if ((rc = ensure_mlp(h, (size_t)M, backward ? 1 : 0))) return rc;
            MlpWeights Wt;
            for (int l = 0; l < SMPC_MAX_LAYERS; l++) { Wt.wf[l] = net.Wfwd[l]; Wt.wb[l] = net.Wbwd[l]; Wt.bias[l] = net.bias[l]; }
            const dim3 grd((M + MLPF_ROWS - 1) / MLPF_ROWS), blk(64);
            if (backward)
                hipLaunchKernelGGL((k_mlp_wave<NQ, true>), grd, blk, 0, s, h->d_desc, M, N, mode, net.act, Wt, d_x, d_p, idx, live, h->d_y.p, d_ev,
                                   compact, h->d_dg[0].p, h->d_dg[1].p, h->d_dg[2].p, cx);
            else
                hipLaunchKernelGGL((k_mlp_wave<NQ, false>), grd, blk, 0, s, h->d_desc, M, N, mode, net.act, Wt, d_x, d_p, idx, live, h->d_y.p,
                                   (double*)nullptr, 0, (float*)nullptr, (float*)nullptr, (float*)nullptr, cx);
            HIPCHK(h, hipGetLastError());
            if (chained) *chained = backward;
            return SMPC_OK;
        }
    }
    if ((rc = ensure_mlp(h, (size_t)M))) return rc;
    hipLaunchKernelGGL((k_nn_features<NQ>), dim3((Mp + 63) / 64), dim3(64), 0, s, h->d_desc, M, Mp, N, mode, d_x,
                       h->d_S.p, idx, live, cx);
    // The layer-by-layer GEMMs (round 4): k_gemm_f32 as ONE-WAVE blocks -- a wavefront of it is self-contained (32 x 64 tile,
    // operands from L2, 90-130 registers, no LDS), so its blocks start on any SIMD with one free slot.  A 128 x 128 LDS-tiled kernel
    // (256-thread blocks: 200 registers per lane on all four SIMDs of one CU at once + 37 KB of LDS), since retired, was 12 % faster
    // alone on the GPU (90 vs 79 TFLOP/s) but in C4's loop its blocks waited for CUs that QP wavefronts keep refilling: 12-14 ms per
    // solve for 1.9 ms of work (profiles/r04_c4_kernel_summary_by_grid.txt).
    const dim3 blk(64), grd(Mp / 32, H / 64);
    hipLaunchKernelGGL((k_gemm_f32<EPI_BIAS_GELU>), grd, blk, 0, s, Mp, H, MLP_KPAD, h->d_S.p, net.Wfwd[0], net.bias[0],
                       (const float*)nullptr, h->d_act[0].p, h->d_dg[0].p, live, net.act);
    for (int l = 1; l + 1 < L; l++)
        hipLaunchKernelGGL((k_gemm_f32<EPI_BIAS_GELU>), grd, blk, 0, s, Mp, H, H, h->d_act[l - 1].p, net.Wfwd[l], net.bias[l],
                           (const float*)nullptr, h->d_act[l].p, h->d_dg[l].p, live, net.act);
    hipLaunchKernelGGL(k_nn_output, dim3((Mp + 3) / 4), dim3(256), 0, s, Mp, H, h->d_act[L - 2].p, h->d_dg[L - 2].p,
                       net.Wbwd[L - 1], net.bias[L - 1], h->d_y.p, h->d_dA.p, live);
    if (backward) {
        float *cur = h->d_dA.p, *nxt = h->d_dB.p;
        for (int l = L - 2; l >= 1; l--) {
            hipLaunchKernelGGL((k_gemm_f32<EPI_MUL>), grd, blk, 0, s, Mp, H, H, cur, net.Wbwd[l], (const float*)nullptr,
                               h->d_dg[l - 1].p, nxt, (float*)nullptr, live, net.act);
            float* t = cur; cur = nxt; nxt = t;
        }
        hipLaunchKernelGGL((k_gemm_f32<EPI_PLAIN>), dim3(Mp / 32, MLP_NPAD / 64), blk, 0, s, Mp, MLP_NPAD, H, cur,
                           net.Wbwd[0], (const float*)nullptr, (const float*)nullptr, h->d_GS.p, (float*)nullptr, live, net.act);
    }
    HIPCHK(h, hipGetLastError());
    return SMPC_OK;
}

// The network's row (value + gradient w.r.t. the state, chain rule and per-node switch included) of every node that carries it:
// into the nodes' linearisation records (compact = 0) or into nn[node][1 + nx] (compact = 1, what the stage builder reads).
template <int NQ>
int launch_nn(smpc_handle* h, int B, const double* d_xg, const double* d_p, double* d_out, int compact) {
    if (h->desc.nn_mode == SMPC_NN_NONE) return SMPC_OK;
    const int N = h->N;
    hipStream_t s = h->stream;
    if (h->net->nlayers == 0) return fail(h, SMPC_ESTATE, "nn_mode != NONE but smpc_set_mlp was not called");
    // row on every node: only the nodes whose per-node switch is on are evaluated (compacted list, mode 3)
    const int mode = h->desc.nn_mode == SMPC_NN_TERMINAL ? 1 : 3;
    const int M = mode == 1 ? B : B * N;
    int rc;
    if (mode == 3) {
        if ((rc = ensure_nn_idx(h, (size_t)M))) return rc;
        hipLaunchKernelGGL(k_nn_compact, dim3((M + 63) / 64), dim3(64), 0, s, M, N, d_p, h->d_nn_idx.p, h->d_nn_cnt);
    }
    bool chained = false;
    if ((rc = run_mlp<NQ>(h, M, mode, N, d_xg, true, rows_of_nodes(N + 1), d_p, d_out, &chained, compact))) return rc;
    if (!chained)
        hipLaunchKernelGGL((k_nn_chain<NQ>), dim3((M + 63) / 64), dim3(64), 0, s, h->d_desc, M, N, mode, d_xg, d_p,
                           h->d_y.p, h->d_GS.p, d_out, mode == 3 ? h->d_nn_idx.p : (const int32_t*)nullptr,
                           mode == 3 ? h->d_nn_cnt : (const int32_t*)nullptr, compact);
    HIPCHK(h, hipGetLastError());
    return SMPC_OK;
}

// f(std::true_type{}, sc) with the handle's scene track when it was set for B instances, else f(std::false_type{}, nullptr): a launcher
// names its kernel and its arguments once, as with with_rows below.  (The SCENE instantiation first: a kernel's place in the code
// object follows its first mention, see ensure_batch.)  off: added to the clock (smpc_loop_post); clocked = false: the kernel
// counts time from 0 (smpc_score_rollout).  A single column needs no time, so the clock is not handed on with T = 1; a forecast
// (smpc_forecast_scene) is laid out from the clock's time on, so it is read from time 0 as well, `off` included.
template <class F> int with_scene(const smpc_handle* h, int B, F&& f, int64_t off = 0, bool clocked = true) {
    if (const double* geom = h->scene.for_batch(B)) {
        if (h->scene_fc) return f(std::true_type{}, SceneSrc{geom, nullptr, h->scene_T, 0});
        return f(std::true_type{}, SceneSrc{geom, clocked && h->scene_T > 1 ? h->scene_clock : nullptr, h->scene_T, off});
    }
    return f(std::false_type{}, (const double*)nullptr);
}

// f(std::true_type{}, md) with the handle's table of instance models when it was set for B instances, else f(std::false_type{}) --
// no argument at all, so that a shared-model kernel is launched with the argument list it always had (ModelSrc, device_model.hpp);
// a launcher takes `auto... md` and hands `md...` on.  The launchers of the kernels that form the controller's dynamics nest it
// inside with_scene.
template <class F> int with_model(const smpc_handle* h, int B, F&& f) {
    if (const ModelSrc table = h->models.for_batch(B)) return f(std::true_type{}, table);
    return f(std::false_type{});
}

// f(rb) with the handle's row-bounds table when it was set for B instances, else f() -- no argument at all, as with_model: the
// launchers of the kernels that read the OCP's row bounds nest it innermost, take `auto... rb` and hand `md..., rb...` on.  (The
// call without the table first: a kernel's place in the code object follows its first mention, and the older ones keep theirs.)
template <class F> int with_row_bounds(const smpc_handle* h, int B, F&& f) {
    const double* table = h->rowb.for_batch(B);
    if (!table) return f();
    return f(table);
}

// The guards of an entry point that evaluates collision rows and runs the network (SlotTag::guard)
int guard_scene_and_context(smpc_handle* h, int B, const char* who) {
    const int rc = h->scene.guard(h, B, who);
    return rc ? rc : h->ctx.guard(h, B, who);
}
// ... and forms the controller's dynamics as well
int guard_scene_context_and_models(smpc_handle* h, int B, const char* who) {
    const int rc = guard_scene_and_context(h, B, who);
    return rc ? rc : h->models.guard(h, B, who);
}

// ... and reads the OCP's own row bounds: the entry points that solve, or state the QP or its merit
int guard_solve_slots(smpc_handle* h, int B, const char* who) {
    const int rc = guard_scene_context_and_models(h, B, who);
    return rc ? rc : h->rowb.guard(h, B, who);
}

// A forecast goes when its world or its horizon does (smpc_forecast_scene): the scene slot if it holds one, and the context if a
// forecast wrote it.  Slots that a setter filled are not touched.
void drop_forecast(smpc_handle* h) {
    if (h->scene_fc) h->scene.clear();
    if (h->ctx_fc) h->ctx.clear();
    h->scene_fc = h->ctx_fc = false;
}

// The reference table of a policy step: the handle's curves (a table per instance) or the caller's shared one (stride 0), or none.
struct TrajSrc {
    const double* p = nullptr;
    long len = 0, stride = 0;
};
int policy_traj_src(smpc_handle* h, int B, const smpc_policy_state* st, TrajSrc* out) {
    int rc;
    if ((rc = h->curves.guard(h, B, "smpc_policy_step"))) return rc;
    if (const double* own = h->curves.held()) {
        if (st->traj)
            return fail(h, SMPC_EINVAL, "smpc_policy_step: st->traj given (traj_len %lld) while instance curves are set (%d instances, "
                        "%lld columns): two sources for one input, clear one", (long long)st->traj_len, h->curves.B, (long long)h->curves_L);
        *out = TrajSrc{own, (long)h->curves_L, 3 * (long)h->curves_L};
        return SMPC_OK;
    }
    if (st->traj) {
        if (st->traj_len < 1) return fail(h, SMPC_EINVAL, "traj_len must be >= 1");
        *out = TrajSrc{st->traj, (long)st->traj_len, 0};
    }
    return SMPC_OK;
}

// the nodes' linearisation records by the thread-per-node kernel, the network's row included (smpc_eval_nodes, and the reference
// set-up of smpc_debug_stage_records; not on the solve path)
template <int NQ>
int launch_eval(smpc_handle* h, int B, const double* d_xg, const double* d_ug, const double* d_p, double* d_ev) {
    const int N = h->N;
    hipStream_t s = h->stream;
    const long n1 = (long)B * (N + 1);
    with_scene(h, B, [&](auto SCENE, auto sc) {
        return with_model(h, B, [&](auto MODEL, auto... md) {
            hipLaunchKernelGGL((k_node_linearise<NQ, SCENE, MODEL>), dim3((unsigned)((n1 + 63) / 64)), dim3(64), 0, s, h->d_desc, B, N, d_xg,
                               d_ug, d_p, d_ev, sc, md...);
            return SMPC_OK;
        });
    });
    HIPCHK(h, hipGetLastError());
    int rc;
    if ((rc = launch_nn<NQ>(h, B, d_xg, d_p, d_ev, 0))) return rc;
    // (this path has no stage builder behind the network pass to hand the row list's counter back at zero: see d_nn_cnt)
    if (h->desc.nn_mode == SMPC_NN_ALL && h->d_nn_cnt) HIPCHK(h, hipMemsetAsync(h->d_nn_cnt, 0, sizeof(int32_t), s));
    return SMPC_OK;
}

// k_qp_ipm's non-temporal variant: -1 (default) by workspace size, 0 / 1 forced (SMPC_QP_NT, A/B runs).  The threshold sits between
// what was measured to lose (a 244 MB sub-batch workspace, three of them in flight) and to win (489 MB, three in flight).
constexpr size_t qp_nt_threshold = (size_t)384 << 20;
static int qp_nt_mode() {
    static const int v = [] { const char* e = getenv("SMPC_QP_NT"); return e ? atoi(e) : -1; }();
    return v;
}

// k_qp_ipm's crew: the wavefronts of a launch as a fraction f of its pairs of instances, G = ceil(f pairs); the G wavefronts take
// the pairs longest-first from a ticket (kernel_qp.hpp).  f = 1 is a wavefront per pair.  Per handle by smpc_set_qp_crew, for the
// process by SMPC_QP_CREW (A/B runs).  The default is the measured one: profiles/qp_crew.txt, DESIGN.md section 4, point 4c.
constexpr double QP_CREW_DEFAULT = 1.0;
static double qp_crew_default() {
    static const double v = [] {
        const char* e = getenv("SMPC_QP_CREW");
        const double f = e ? atof(e) : QP_CREW_DEFAULT;
        return f > 0.0 && f <= 1.0 ? f : QP_CREW_DEFAULT;
    }();
    return v;
}
static int qp_crew_waves(const smpc_handle* h, int B) {
    const int pairs = (B + 1) / 2;
    if (h->qp_crew_waves > 0) return h->qp_crew_waves < pairs ? h->qp_crew_waves : pairs;
    const double f = h->qp_crew > 0.0 ? h->qp_crew : qp_crew_default();
    const int g = (int)ceil(f * pairs);
    return g < 1 ? 1 : (g > pairs ? pairs : g);
}

// f(std::integral_constant<int, MR>{}) with the handle's row count as the kernels' compile-time constant: the shipped geometries
// have 6 rows (the reference's six capsule pairs, config.yaml:205-216) or 4 (config_fr7.yaml); any other count takes the
// runtime-row-count instantiation, MR = -1
template <class F> int with_rows(const smpc_handle* h, F&& f) {
    switch (h->desc.n_rows) {
    case 6: return f(std::integral_constant<int, 6>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, -1>{});
    }
}

// Room for the per-instance bounds of B instances, zeroed when grown if asked: lo in the buffer's first half, hi in its second (a
// half keeps its place, and what it holds, whatever B a buffer that is large enough serves next)
int ensure_instance_bounds(smpc_handle* h, int B, bool zero) { return h->bounds.room(h, (size_t)2 * B * (h->N + 1) * 2 * h->desc.nq, zero); }
double* instance_hi(const smpc_handle* h) { return h->bounds.d.p ? h->bounds.d.p + h->bounds.d.cap / (2 * sizeof(double)) : nullptr; }

// the stage bounds the set-up reads: per instance (RealReceding) when they were given for this batch size, else the shared ones
struct StageBounds {
    const double *lo, *hi;
    long stride;
};
StageBounds stage_bounds(const smpc_handle* h, int B) {
    if (const double* lo = h->bounds.for_batch(B)) return {lo, instance_hi(h), (long)(h->N + 1) * 2 * h->desc.nq};
    return {h->d_lo.p, h->d_hi.p, 0L};
}

// everything of a solve before the interior point: the network pass, then the stage records of the QP workspace by the
// lane-cooperative stage builder (kernel_build.hpp)
template <int NQ>
int launch_stage_records(smpc_handle* h, int B, const double* x0, const double* xg, const double* ug, const double* p, bool timed) {
    int rc;
    if ((rc = launch_nn<NQ>(h, B, xg, p, h->d_nn.p, h->desc.nn_mode == SMPC_NN_TERMINAL ? 2 : 1))) return rc;
    if (timed) HIPCHK(h, hipEventRecord(h->ev_t[1], h->stream));
    const StageBounds bd = stage_bounds(h, B);
    const long nodes = (long)B * (h->N + 1);
    const dim3 grd((unsigned)((nodes + 64 / SB_G - 1) / (64 / SB_G))), blk(64);
    const double* nn = h->desc.nn_mode != SMPC_NN_NONE ? h->d_nn.p : nullptr;
    int32_t* const zero_cnt = h->desc.nn_mode == SMPC_NN_ALL ? h->d_nn_cnt : nullptr;     // (the builder hands the list's counter back at zero)
    with_rows(h, [&](auto MR) {
        return with_scene(h, B, [&](auto SCENE, auto sc) {
            return with_model(h, B, [&](auto MODEL, auto... md) {
                return with_row_bounds(h, B, [&](auto... rb) {
                    hipLaunchKernelGGL((k_stage_build<NQ, MR, SCENE, MODEL>), grd, blk, 0, h->stream, h->d_desc, B, h->N, x0, xg, ug, p, bd.lo,
                                       bd.hi, h->d_zl.p, nn, h->d_ws.p, bd.stride, h->d_active, zero_cnt, sc, md..., rb...);
                    return SMPC_OK;
                });
            });
        });
    });
    HIPCHK(h, hipGetLastError());
    // (ev4 ends the set-up of the QP, which the builder has done: smpc_get_qp_timing's ms2[0], the gap from ev2 to ev4, is ~0)
    if (timed) { HIPCHK(h, hipEventRecord(h->ev_t[2], h->stream)); HIPCHK(h, hipEventRecord(h->ev_t[4], h->stream)); }
    return SMPC_OK;
}

// The same stage records by the thread-per-node kernels of rounds 1-3 (k_node_linearise -> network pass -> k_qp_setup): not on
// the solve path, only the independent reference that smpc_debug_stage_records (path 0) builds them with
template <int NQ>
int launch_stage_records_per_node(smpc_handle* h, int B, const double* x0, const double* xg, const double* ug, const double* p) {
    int rc;
    if ((rc = launch_eval<NQ>(h, B, xg, ug, p, h->d_ev.p))) return rc;
    const StageBounds bd = stage_bounds(h, B);
    const int tiles = (int)ev_tiles((size_t)B * (h->N + 1));
    with_rows(h, [&](auto MR) {
        return with_row_bounds(h, B, [&](auto... rb) {
            hipLaunchKernelGGL((k_qp_setup<NQ, MR>), dim3(tiles), dim3(32 * EV_TILE), 0, h->stream, h->d_desc, B, h->N, x0, xg, ug, p, bd.lo,
                               bd.hi, h->d_zl.p, h->d_ev.p, h->d_ws.p, bd.stride, h->d_active, rb...);
            return SMPC_OK;
        });
    });
    HIPCHK(h, hipGetLastError());
    return SMPC_OK;
}

// k_qp_ipm_wg (kernel_qp_wg.hpp), the latency form of the interior-point solve -- one workgroup per instance: -1 (default) chosen by
// batch size, 0 never, 1 whenever its LDS fits (SMPC_QP_WG; smpc_set_qp_mode per handle).  Built with 8 half-wavefronts per
// workgroup (four wavefronts, one per SIMD: one workgroup per CU -- up to qp_wg_full_batch instances run in one round) and with 4
// (two wavefronts: two workgroups per CU, the stage-parallel phases take twice the rounds -- 512 instances in one round, up to
// qp_wg_max_batch = 1024 in one launch whose later workgroups start as the first ones retire).  Above that k_qp_ipm's two instances per
// wavefront use the chip better (per step, latency form against k_qp_ipm: 0.99 ms against 2.16 at 512 instances, 1.37 against 2.27 at
// 1024 as two sub-batches of 512, 2.06 against 2.46 at 1536 as three; from 2048 on k_qp_ipm wins -- DESIGN.md section 4c).  A handle
// only sees its own launch: a caller that spreads ONE batch over several handles should pick the form from the total (bench.py does:
// the latency form up to 1536 instances per GPU in sub-batches of at most 512).
#ifndef QP_WG_FULL_BATCH
#define QP_WG_FULL_BATCH 256
#endif
#ifndef QP_WG_MAX_BATCH
#define QP_WG_MAX_BATCH 1024
#endif
static int qp_wg_mode() {
    static const int v = [] { const char* e = getenv("SMPC_QP_WG"); return e ? atoi(e) : -1; }();
    return v;
}
static int qp_wg_max_batch() {
    static const int v = [] { const char* e = getenv("SMPC_QP_WG_MAX_BATCH"); return e ? atoi(e) : QP_WG_MAX_BATCH; }();
    return v;
}
static int qp_wg_full_batch() {
    static const int v = [] { const char* e = getenv("SMPC_QP_WG_FULL_BATCH"); return e ? atoi(e) : QP_WG_FULL_BATCH; }();
    return v;
}
constexpr size_t QP_WG_LDS_LIMIT = 160 * 1024 - 512;     // one CU's LDS less the kernel's static tables

// half-wavefronts per workgroup for a launch of B instances (0: the latency form is not to be used)
template <int NQ> int qp_wg_choice(const smpc_handle* h, int B) {
    const int mode = h->qp_mode >= -1 ? h->qp_mode : qp_wg_mode();
    if (mode == 0) return 0;
    if (mode < 0 && B > qp_wg_max_batch()) return 0;
    const auto fits = [&](int nhw) { return (size_t)WgLds<NQ>(h->N, h->desc.n_rows, nhw).total * sizeof(double) <= QP_WG_LDS_LIMIT; };
    if (B <= qp_wg_full_batch() && fits(8)) return 8;
    return fits(4) ? 4 : 0;
}

// (the records and the LDS limit were set up by ensure_batch)
template <int NQ, int NHW>
int launch_qp_wg(smpc_handle* h, int B, const double* x0, const double* xg, const double* ug, double* xo, double* uo, int32_t* st,
                 int32_t* it) {
    if (h->d_hrec.cap < sizeof(double) * B * (h->N + 1) * HRecLayout<NQ>::SIZE)
        return fail(h, SMPC_ESTATE, "latency-form records not grown for %d instances", B);
    const size_t lds = (size_t)WgLds<NQ>(h->N, h->desc.n_rows, NHW).total * sizeof(double);
    return with_rows(h, [&](auto MR) {
        hipLaunchKernelGGL((k_qp_ipm_wg<NQ, MR, NHW>), dim3(B), dim3(32 * NHW), lds, h->stream, h->d_desc, B, h->N, x0, xg, ug, h->d_ws.p,
                           h->d_hrec.p, xo, uo, st, it, h->d_last_it.p, h->d_active, h->d_ord_hist.p);
        return SMPC_OK;
    });
}

// raises k_qp_ipm_wg's dynamic-LDS limit: once per handle = per device, nq and row count, and half-wave count.  The kernel may use a
// whole CU's LDS -- always the same value, so a handle with a short horizon never lowers the limit under one with a long horizon.
template <int NQ, int NHW> int raise_qp_wg_lds_limit(smpc_handle* h) {
    if (h->wg_lds_raised[NHW == 8 ? 0 : 1]) return SMPC_OK;
    const int rc = with_rows(h, [&](auto MR) {
        HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_qp_ipm_wg<NQ, MR, NHW>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)QP_WG_LDS_LIMIT));
        return SMPC_OK;
    });
    h->wg_lds_raised[NHW == 8 ? 0 : 1] = rc == SMPC_OK;
    return rc;
}

// the latency form's records and LDS limit, for a launch of B instances that takes it (ensure_batch)
template <int NQ> int ensure_qp_wg(smpc_handle* h, int B) {
    const int nhw = qp_wg_choice<NQ>(h, B);
    if (nhw == 0) return SMPC_OK;
    int rc;
    if ((rc = h->d_hrec.reserve(h, "latency-form records", sizeof(double) * B * (h->N + 1) * HRecLayout<NQ>::SIZE))) return rc;
    return nhw == 8 ? raise_qp_wg_lds_limit<NQ, 8>(h) : raise_qp_wg_lds_limit<NQ, 4>(h);
}

template <int NQ>
int launch_solve(smpc_handle* h, int B, const double* x0, const double* xg, const double* ug, const double* p,
                 double* xo, double* uo, int32_t* st, int32_t* it) {
    int rc;
    h->timing_now = false;
    if (h->timing) {
        // a solve that is being captured into a hipGraph records nothing: every replay would re-record the one slot it captured
        h->timing_now = !capturing(h);
    }
    const bool timed = h->timing_now;
    if (timed) {
        h->ev_cur = (h->ev_cur + 1) % smpc_handle::EV_RING;
        h->ev_t = h->ev_sets[h->ev_cur];
        h->ev_complete[h->ev_cur] = false;      // (an error return below leaves the slot invalid, not stale)
        h->timed_count++;
        HIPCHK(h, hipEventRecord(h->ev_t[0], h->stream));
    }
    if ((rc = launch_stage_records<NQ>(h, B, x0, xg, ug, p, timed))) return rc;
    const int wg_nhw = qp_wg_choice<NQ>(h, B);
    const bool wg = wg_nhw > 0;
    const int32_t* order = nullptr;
    if (h->order_B == B && B > 1 && !wg) {
        hipLaunchKernelGGL(k_order_by_iters, dim3((B + ORD_PER_BLOCK - 1) / ORD_PER_BLOCK), dim3(64), 0, h->stream, B, h->d_last_it.p,
                           h->d_order.p, h->d_ord_hist.p, h->d_ord_hist.p + 256, h->d_ord_hist.p + 512);
        order = h->d_order.p;
    } else {
        // (no order this time: the histogram k_qp_ipm adds to must hold this solve alone when the next one sorts by it)
        HIPCHK(h, hipMemsetAsync(h->d_ord_hist.p, 0, 520 * sizeof(int32_t), h->stream));
    }
    unsigned long long* wstat = nullptr;
    if (timed && h->timing == 1) {      // (timing mode 2: events only, no in-kernel load-balance probe)
        const unsigned long long init[4] = {0ull, ~0ull, 0ull, 0ull};     // (d_wstat: smpc_enable_timing)
        HIPCHK(h, hipMemcpyAsync(h->d_wstat.p, init, sizeof(init), hipMemcpyHostToDevice, h->stream));
        wstat = h->d_wstat.p;
    }
    // non-temporal workspace accesses once this launch's workspace is well beyond the Infinity Cache (kernel_qp.hpp, k_qp_ipm)
    if (wg) {
        if ((rc = wg_nhw == 8 ? launch_qp_wg<NQ, 8>(h, B, x0, xg, ug, xo, uo, st, it) : launch_qp_wg<NQ, 4>(h, B, x0, xg, ug, xo, uo, st, it))) return rc;
    } else {
        const bool nt = qp_nt_mode() < 0 ? ws_doubles_per_instance(h, h->N) * sizeof(double) * (size_t)B >= qp_nt_threshold : qp_nt_mode() > 0;
        with_rows(h, [&](auto MR) {
            const auto launch = [&](auto NT) {
                // (the pair ticket is zero here: cleared with the histogram, by k_order_by_iters or the memset above)
                hipLaunchKernelGGL((k_qp_ipm<NQ, MR, NT>), dim3(qp_crew_form<NQ, MR>() ? qp_crew_waves(h, B) : (B + 1) / 2), dim3(64), 0, h->stream, h->d_desc, B, h->N, x0, xg, ug,
                                   h->d_ws.p, xo, uo, st, it, order, h->d_last_it.p, wstat, h->d_active, h->d_ord_hist.p, h->d_ord_hist.p + 513);
                return SMPC_OK;
            };
            if constexpr (MR < 0) return launch(std::false_type{});      // (the runtime-row-count instantiation is not built twice)
            else return nt ? launch(std::true_type{}) : launch(std::false_type{});
        });
    }
    h->order_B = B;
    HIPCHK(h, hipGetLastError());
    if (timed) {
        HIPCHK(h, hipEventRecord(h->ev_t[3], h->stream));
        h->ev_complete[h->ev_cur] = true;
        h->timed = 1;
    }
    return SMPC_OK;
}

// The check bounds of the state tests (h->chk): [x_min | x_max | row_lb | row_ub]
struct ChkBlock { double *x_min, *x_max, *row_lb, *row_ub; size_t doubles; };
ChkBlock chk_block(double* base, int nq) {
    Carve m = dense(base);
    ChkBlock b{};
    b.x_min = m.take<double>(2 * nq);
    b.x_max = m.take<double>(2 * nq);
    b.row_lb = m.take<double>(SMPC_MAX_ROWS);
    b.row_ub = m.take<double>(SMPC_MAX_ROWS);
    b.doubles = m.off / sizeof(double);
    return b;
}
int upload_check_bounds(smpc_handle* h, const double* x_min, const double* x_max, const double* row_lb_chk,
                        const double* row_ub_chk) {
    const int nq = h->desc.nq, nr = h->desc.n_rows;
    std::vector<double> img(chk_block(nullptr, nq).doubles, 0.0);
    const ChkBlock b = chk_block(img.data(), nq);
    put(b.x_min, x_min, 2 * nq);
    put(b.x_max, x_max, 2 * nq);
    put(b.row_lb, row_lb_chk, nr);
    put(b.row_ub, row_ub_chk, nr);
    return h->chk.upload(h, img);
}

// state test (+ safe-set test if d_nn) of B trajectories of n_nodes nodes on the device, against the uploaded check bounds;
// collision rows on the leading coll_nodes nodes only.  scene_off: node k sits at time clock + scene_off + k of a scene track (1 for
// smpc_loop_post, whose one node is the plant's next state).
int check_nodes_dev(smpc_handle* h, int B, int n_nodes, const double* d_x, double tol_x, int coll_nodes, double alpha,
                    double tol_safe, int32_t* d_ok, int32_t* d_nn, bool nn_listed = false, bool ok_prefilled = false,
                    int64_t scene_off = 0) {
    hipStream_t s = h->stream;
    const size_t M = (size_t)B * n_nodes;
    const ChkBlock c = chk_block(h->chk.d.p, h->desc.nq);
    // verdicts start at "ok", stream-ordered (smpc_policy_step: an earlier kernel of the step has done it)
    if (!ok_prefilled) HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)d_ok, 1, (size_t)B, s));
    // (one wavefront per block throughout the small kernels: a multi-wave block needs room on several SIMDs of ONE CU at the
    //  same moment, and next to resident QP wavefronts -- 256 registers each, two fill a SIMD -- it waited for that up to a
    //  millisecond: k_policy_post, six blocks of four waves, averaged 131 us in the three-stream loop; rocprofv3, round 3)
    const dim3 grd((unsigned)((M + 63) / 64)), blk(64);
    int rc;
    const auto launch = [&](auto SCENE, auto sc) {
        return with_nq(h, [&](auto NQ) {
            hipLaunchKernelGGL((k_check_nodes<NQ, SCENE>), grd, blk, 0, s, h->d_desc, B, n_nodes, d_x, c.x_min, c.x_max, tol_x, c.row_lb,
                               c.row_ub, d_ok, coll_nodes, sc);
            return SMPC_OK;
        });
    };
    // the plant's next state (smpc_loop_post: scene_off = 1) meets the WORLD while one is set (its caller has guarded B), clocked
    // like a scene track; every other test reads the scene slot, which is what the controller believes
    const double* world = scene_off == 1 ? h->world.held() : nullptr;
    if ((rc = world ? launch(std::true_type{}, SceneSrc{world, h->world_T > 1 ? h->scene_clock : nullptr, h->world_T, scene_off})
                    : with_scene(h, B, launch, scene_off)))
        return rc;
    HIPCHK(h, hipGetLastError());
    if (d_nn) {
        // nn_listed: only the nodes in h->d_nn_idx (length on the device, h->d_nn_cnt) are evaluated; their verdicts land at the
        // nodes' own positions of d_nn, the rest of d_nn is left as it is
        if ((rc = with_nq(h, [&](auto NQ) { return run_mlp<NQ>(h, (int)M, nn_listed ? 3 : 0, 0, d_x, false, rows_of_nodes(n_nodes)); }))) return rc;
        const int32_t* li = nn_listed ? h->d_nn_idx.p : nullptr;
        const int32_t* lc = nn_listed ? h->d_nn_cnt : nullptr;
        if ((rc = with_nq(h, [&](auto NQ) {
                 hipLaunchKernelGGL((k_check_nn<NQ>), grd, blk, 0, s, h->d_desc, (int)M, d_x, alpha, tol_safe, h->d_y.p, d_nn, li, lc);
                 return SMPC_OK;
             })))
            return rc;
        HIPCHK(h, hipGetLastError());
    }
    return SMPC_OK;
}

// scratch of the policy entry points: smpc_policy_step's verdicts and masks, then smpc_loop_post's next state of the plant and its
// verdicts (one layout for both: the two are enqueued one after the other on the handle's stream)
struct PolScratch {
    int32_t *ok, *safe, *acc;   // state_ok [B] | safe [B][N+1] | accept [B]
    uint8_t* act;               // [B]
    double* xn;                 // [B][nx]
    int32_t* okn;               // [B]
    size_t bytes;
};
PolScratch pol_layout(char* base, int B, int N, int nx) {
    Carve m{base};
    PolScratch w{};
    w.ok = m.take<int32_t>(B);
    w.safe = m.take<int32_t>((size_t)B * (N + 1));
    w.acc = m.take<int32_t>(B);
    w.act = m.take<uint8_t>(B);
    w.xn = m.take<double>((size_t)B * nx);
    w.okn = m.take<int32_t>(B);
    w.bytes = m.off;
    return w;
}
int policy_scratch(smpc_handle* h, int B, PolScratch* w) {
    const int nx = 2 * h->desc.nq;
    int rc;
    if ((rc = h->d_polw.reserve(h, "policy scratch", pol_layout(nullptr, B, h->N, nx).bytes))) return rc;
    *w = pol_layout(h->d_polw.p, B, h->N, nx);
    return SMPC_OK;
}

// scratch of smpc_rollout_batch for the n instances one handle steps: the policy's fails / accept counters (kept in the handle: the
// device path does not synchronise) and the solve's outputs
struct RollScratch {
    int32_t *fails, *accept, *it;
    double *xo, *uo;
    size_t bytes;
};
RollScratch roll_layout(char* base, int n, int N, int nq) {
    Carve m{base};
    RollScratch r{};
    r.fails = m.take<int32_t>(n);
    r.accept = m.take<int32_t>(n);
    r.xo = m.take<double>((size_t)n * (N + 1) * 2 * nq);
    r.uo = m.take<double>((size_t)n * N * nq);
    r.it = m.take<int32_t>(n);
    r.bytes = m.off;
    return r;
}

// Worker handles of smpc_rollout_batch: same problem, own stream and workspaces, the parent's network (smpc_handle::net).  What a
// worker takes from its parent it takes here, on every call: no setter pushes a value to the workers.
int rollout_workers(smpc_handle* h, int n) {
    while ((int)h->kids.size() < n) {
        smpc_handle* k = nullptr;
        int rc = smpc_create(&h->desc, h->device, &k);
        if (rc) return fail(h, rc, "rollout worker: %s", smpc_last_error(nullptr));
        h->kids.push_back(k);
    }
    for (int i = 0; i < n; i++) {
        smpc_handle* k = h->kids[i];
        int rc;
        if (k->N != h->N && (rc = smpc_set_horizon(k, h->N))) return fail(h, rc, "rollout worker: %s", k->err);
        k->net = h->net;                // (with the weights goes the default context; a worker holds no instance context)
        k->qp_mode = h->qp_mode;
        k->qp_crew = h->qp_crew;
        k->qp_crew_waves = h->qp_crew_waves;
        // stage bounds and slack weights follow the parent (small; stream-ordered on the worker's stream)
        const size_t nb = (size_t)(h->N + 1) * 2 * h->desc.nq;
        HIPCHK(h, hipMemcpyAsync(k->d_lo.p, h->d_lo.p, nb * sizeof(double), hipMemcpyDeviceToDevice, k->stream));
        HIPCHK(h, hipMemcpyAsync(k->d_hi.p, h->d_hi.p, nb * sizeof(double), hipMemcpyDeviceToDevice, k->stream));
        if (h->d_zl.p) {
            if ((rc = k->d_zl.reserve(k, "slack weights", sizeof(double) * (h->N + 1)))) return fail(h, rc, "rollout worker: %s", k->err);
            HIPCHK(h, hipMemcpyAsync(k->d_zl.p, h->d_zl.p, sizeof(double) * (h->N + 1), hipMemcpyDeviceToDevice, k->stream));
        } else if (k->d_zl.p) {
            HIPCHK(h, hipStreamSynchronize(k->stream));
            k->d_zl.release();
        }
    }
    return SMPC_OK;
}

// ---- SMPC_POLICY_PARALLEL (kernels_policy.hpp, k_par_*) ------------------------------------------------------------------------
// the candidate block for B instances at horizon N (K = N - 1 candidates per instance in phase 2, S = B * K slots)
struct ParScratch {
    double *p1, *x0, *xg, *ug, *p, *xo, *uo;
    int32_t *st, *it, *ok, *safe, *list, *pos, *n_open;
    uint8_t* active;
    size_t bytes;
};
ParScratch par_layout(char* base, int B, int N, int nq) {
    const size_t S = (size_t)B * (N - 1), nx = 2 * (size_t)nq;
    Carve m{base};
    ParScratch c{};
    c.p1 = m.take<double>((size_t)B * (N + 1) * SMPC_NP);
    c.x0 = m.take<double>(S * nx);
    c.xg = m.take<double>(S * (N + 1) * nx);
    c.ug = m.take<double>(S * N * nq);
    c.p = m.take<double>(S * (N + 1) * SMPC_NP);
    c.xo = m.take<double>(S * (N + 1) * nx);
    c.uo = m.take<double>(S * N * nq);
    c.st = m.take<int32_t>(S);
    c.it = m.take<int32_t>(S);
    c.ok = m.take<int32_t>(S);
    c.safe = m.take<int32_t>(S * (N + 1));
    c.list = m.take<int32_t>(B);
    c.pos = m.take<int32_t>(B);
    c.n_open = m.take<int32_t>(1);
    c.active = m.take<uint8_t>(S);
    c.bytes = m.off;
    return c;
}

int ensure_batch(smpc_handle* h, int B, bool with_ev = true);

// everything a parallel step needs beyond what every policy step has: the candidate block, the solve path's scratch (QP workspace,
// network-row records) for max(B, S) instances, the network lists for S * (N + 1) nodes.  Grown on the first step of a batch size.
int ensure_parallel(smpc_handle* h, int B) {
    const int N = h->N;
    const long S = (long)B * (N - 1);
    const ParScratch need = par_layout(nullptr, B, N, h->desc.nq);
    const size_t ws = ws_doubles_per_instance(h, N) * sizeof(double) * (size_t)(S > B ? S : B);
    int rc = S > INT32_MAX / (N + 1) ? SMPC_EINVAL : SMPC_OK;
    if (!rc) rc = h->d_par.reserve(h, "parallel candidate buffers", need.bytes, true);
    if (!rc && S > 0) rc = ensure_batch(h, (int)(S > B ? S : B), false);
    if (!rc && S > 0) rc = ensure_nn_idx(h, (size_t)S * (N + 1));
    if (rc == SMPC_EINVAL || rc == SMPC_ENOMEM)
        return fail(h, rc, "parallel policy: candidate scratch for B * (N - 1) = %ld instances could not be allocated: %.2f GB of QP "
                    "workspace + %.2f GB of candidate buffers (B = %d, N = %d)", S, ws / 1e9, need.bytes / 1e9, B, N);
    return rc;
}

// ParallelController.step (controller.py:567-644) for the stepping instances, enqueue-only.  Phase 1: candidate N of every stepping
// instance -- the htwa OCP under per-node switching -- into the instance's own x_temp / u_temp / status / qp_iter, its state test and
// its safe-set test at nodes r..N.  Phase 2: candidates N-1 .. 1 of the instances phase 1 left open, as one launch over the dense
// candidate list (dead slots skipped), tested the same way.  Then k_par_select (selection and automaton) and provideControl.
int policy_step_parallel(smpc_handle* h, int B, const smpc_policy_params* par, const smpc_policy_state* st, const double* x,
                         const uint8_t* stepping, const double* u_other, double* u_out, uint8_t* abort_out, int32_t* any_abort,
                         int32_t* d_ok, int32_t* d_safe, int32_t* d_acc, uint8_t* d_act) {
    const int N = h->N, nq = h->desc.nq, nx = 2 * nq, K = N - 1;
    const long S = (long)B * K;
    hipStream_t s = h->stream;
    int rc;
    if ((rc = ensure_parallel(h, B))) return rc;
    if ((rc = ensure_nn_idx(h, (size_t)B * (N + 1)))) return rc;
    TrajSrc tr;
    if ((rc = policy_traj_src(h, B, st, &tr))) return rc;
    const ParScratch c = par_layout(h->d_par.p, B, N, nq);
    const dim3 blk(64);
    const auto grid = [](long n) { return dim3((unsigned)((n + 63) / 64)); };
    // guessCorrection; also resets *any_abort and presets the state-test verdicts of phase 1
    hipLaunchKernelGGL(k_guess_correction, grid((long)B * nq), blk, 0, s, B, N, nq, h->desc.dt, st->x_guess, st->u_guess, stepping,
                       any_abort, d_ok);
    if (tr.p)            // controller.py:153-156, into the instance's own p (what solve() writes there)
        hipLaunchKernelGGL(k_policy_traj, grid((long)B * (N + 1)), blk, 0, s, B, N, stepping, st->current_step, tr.p, tr.len, tr.stride,
                           st->p);
    hipLaunchKernelGGL(k_par_fanout1, grid((long)B * (N + 1)), blk, 0, s, B, N, stepping, st->p, c.p1, c.n_open);
    HIPCHK(h, hipGetLastError());
    const int coll = par->collision_first_node ? 1 : N + 1;
    // The network kernel (run_mlp) is chosen by the rows of the statement that solves all B * N candidates at once -- B * N * N in the
    // solve, B * N * (N + 1) in the safe-set test -- so that both schedules take the same kernel and give the same numbers
    const long rows_solve = (long)B * N * N, rows_test = (long)B * N * (N + 1);
    h->d_active = stepping;
    h->mlp_rows_hint = rows_solve;
    rc = with_nq(h, [&](auto NQ) { return launch_solve<NQ>(h, B, x, st->x_guess, st->u_guess, c.p1, st->x_temp, st->u_temp, st->status, st->qp_iter); });
    h->d_active = nullptr;
    if (rc) { h->mlp_rows_hint = 0; return rc; }
    h->mlp_rows_hint = rows_test;
    hipLaunchKernelGGL(k_par_safe_list, grid((long)B * (N + 1)), blk, 0, s, B, N, K, stepping, (const int32_t*)nullptr,
                       (const int32_t*)nullptr, st->r, st->status, h->d_nn_idx.p, h->d_nn_cnt);
    if ((rc = check_nodes_dev(h, B, N + 1, st->x_temp, par->tol_x, coll, par->alpha, par->tol_safe, d_ok, d_safe, true, true))) {
        h->mlp_rows_hint = 0;
        return rc;
    }
    hipLaunchKernelGGL(k_par_compact, grid(B), blk, 0, s, B, N, stepping, st->r, st->status, d_ok, d_safe, c.list, c.pos, c.n_open,
                       h->d_nn_cnt);
    if (K > 0) {
        // phase 2 over the candidate capacity S: the live slots are the first *n_open * K.  The QP form follows S (or the pinned mode),
        // never the live count, which the host does not see.
        hipLaunchKernelGGL(k_par_fanout2, grid(S * (N + 1)), blk, 0, s, (int)S, N, nq, c.list, c.n_open, x, st->x_guess, st->u_guess,
                           st->p, c.x0, c.xg, c.ug, c.p, c.active, c.ok);
        HIPCHK(h, hipGetLastError());
        h->d_active = c.active;
        h->mlp_rows_hint = rows_solve;
        rc = with_nq(h, [&](auto NQ) { return launch_solve<NQ>(h, (int)S, c.x0, c.xg, c.ug, c.p, c.xo, c.uo, c.st, c.it); });
        h->d_active = nullptr;
        if (rc) { h->mlp_rows_hint = 0; return rc; }
        h->mlp_rows_hint = rows_test;
        hipLaunchKernelGGL(k_par_safe_list, grid(S * (N + 1)), blk, 0, s, (int)S, N, K, stepping, c.list, c.n_open, st->r, c.st,
                           h->d_nn_idx.p, h->d_nn_cnt);
        const ChkBlock cb = chk_block(h->chk.d.p, nq);
        const long M = S * (N + 1);
        rc = with_nq(h, [&](auto NQ) {
            hipLaunchKernelGGL((k_par_check_state<NQ>), grid(M), blk, 0, s, h->d_desc, (int)S, N, c.n_open, c.xo, cb.x_min, cb.x_max, par->tol_x,
                               cb.row_lb, cb.row_ub, c.st, c.ok, coll);
            HIPCHK(h, hipGetLastError());
            if (const int e = run_mlp<NQ>(h, (int)M, 3, 0, c.xo, false, rows_of_nodes(N + 1))) return e;
            hipLaunchKernelGGL((k_check_nn<NQ>), grid(M), blk, 0, s, h->d_desc, (int)M, c.xo, par->alpha, par->tol_safe, h->d_y.p, c.safe,
                               h->d_nn_idx.p, h->d_nn_cnt);
            HIPCHK(h, hipGetLastError());
            return SMPC_OK;
        });
        if (rc) { h->mlp_rows_hint = 0; return rc; }
    }
    h->mlp_rows_hint = 0;
    hipLaunchKernelGGL(k_par_select, grid(B), blk, 0, s, B, N, nq, stepping, d_ok, d_safe, c.pos, c.st, c.it, c.ok, c.safe, c.xo, c.uo,
                       st->x_temp, st->u_temp, st->status, st->qp_iter, st->x_guess, st->fails, st->current_step, st->r, st->x_viable,
                       d_acc, d_act, abort_out, any_abort, h->d_nn_cnt);
    hipLaunchKernelGGL(k_provide_control, grid((long)B * (nx + nq)), blk, 0, s, B, N, nq, d_acc, st->x_temp, st->u_temp, st->x_guess,
                       st->u_guess, u_out, stepping, d_act, u_other);
    HIPCHK(h, hipGetLastError());
    return SMPC_OK;
}

// The solve path's per-batch buffers for B instances.  with_ev = false: the solve path only (SMPC_POLICY_PARALLEL's candidate batch),
// which never reads the linearisation records d_ev -- 2.6 KB per node, 10 GB for the candidates of 4096 instances at N = 30 -- so
// they are not grown for it.  (Defined after the solve path on purpose: a kernel's place in the code object follows the first
// mention of it in this file, and ensure_qp_wg must not be the first to name k_qp_ipm_wg.)
int ensure_batch(smpc_handle* h, int B, bool with_ev) {
    const size_t nodes = (size_t)B * (h->N + 1);
    const size_t nn_nodes = h->desc.nn_mode == SMPC_NN_NONE ? 0 : (h->desc.nn_mode == SMPC_NN_TERMINAL ? (size_t)B : nodes);
    int rc;
    if ((with_ev && (rc = h->d_ev.reserve(h, "linearisation records", sizeof(double) * ev_tiles(nodes) * EV_TILE * EV_D))) ||
        (rc = h->d_ws.reserve(h, "QP workspace", sizeof(double) * ws_doubles_per_instance(h, h->N) * B)) ||
        // (entries beyond n_dof_safe_set are never written and must read as zero)
        (rc = h->d_nn.reserve(h, "network rows", sizeof(double) * nn_nodes * (1 + 2 * h->desc.nq), true)) ||
        (rc = h->d_order.reserve(h, "dispatch order", sizeof(int32_t) * B)))
        return rc;
    const size_t had = h->d_last_it.cap;
    rc = h->d_last_it.reserve(h, "iteration counts", sizeof(int32_t) * B);
    if (h->d_last_it.cap != had) h->order_B = 0;     // (a new or freed d_last_it holds no iterations; a refused growth keeps them)
    if (rc || (rc = h->d_ord_hist.reserve(h, "iteration histogram", sizeof(int32_t) * 520, true))) return rc;
    return with_nq(h, [&](auto NQ) { return ensure_qp_wg<NQ>(h, B); });
}

// ---- SQP with merit backtracking (kernels_sqp.hpp) -----------------------------------------------------------------------------
// scratch of smpc_sqp_batch and smpc_merit_terms for B instances: the QP's solution and the step, the trial points' states (what
// the network pass reads), the line search's per-instance state
struct SqpScratch {
    double *xs, *us, *dx, *du, *xt, *step, *m0t, *mt, *alpha, *m0, *Dd;
    int32_t *st, *it, *pos, *n_open;
    uint8_t *act, *settled, *trial;
    size_t bytes;
};
SqpScratch sqp_layout(char* base, int B, int N, int nq, bool full) {
    const size_t nX = (size_t)B * (N + 1) * 2 * nq, nU = (size_t)B * N * nq;
    Carve m{base};
    SqpScratch w{};
    w.xt = m.take<double>(nX);
    w.pos = m.take<int32_t>((size_t)B * (N + 1));
    if (full) {
        w.xs = m.take<double>(nX);
        w.us = m.take<double>(nU);
        w.dx = m.take<double>(nX);
        w.du = m.take<double>(nU);
        w.step = m.take<double>(B);
        w.m0t = m.take<double>((size_t)3 * B);
        w.mt = m.take<double>((size_t)3 * B);
        w.alpha = m.take<double>(B);
        w.m0 = m.take<double>(B);
        w.Dd = m.take<double>(B);
        w.st = m.take<int32_t>(B);
        w.it = m.take<int32_t>(B);
        w.n_open = m.take<int32_t>(1);
        w.act = m.take<uint8_t>(B);
        w.settled = m.take<uint8_t>(B);
        w.trial = m.take<uint8_t>(B);
    }
    w.bytes = m.off;
    return w;
}
int sqp_scratch(smpc_handle* h, int B, bool full, SqpScratch* w) {
    int rc;
    if ((rc = h->d_sqp.reserve(h, "SQP scratch", sqp_layout(nullptr, B, h->N, h->desc.nq, full).bytes))) return rc;
    *w = sqp_layout(h->d_sqp.p, B, h->N, h->desc.nq, full);
    return SMPC_OK;
}

// {f, viol, gd} of the instances whose mask byte is set, at (x + alpha dx, u + alpha du): the forward-only network pass on the
// nodes that carry the safe-set row (listed by k_sqp_nn_list, so that masked-out instances cost no network rows), then k_merit.
// The list's counter goes back to zero behind the chain (see d_nn_cnt).
template <int NQ>
int launch_merit(smpc_handle* h, int B, const SqpScratch& w, const double* x0, const double* x, const double* u, const double* p,
                 const double* dx, const double* du, const double* alpha, const uint8_t* mask, double* out) {
    const int N = h->N;
    hipStream_t s = h->stream;
    const long nodes = (long)B * (N + 1);
    const float* y = nullptr;
    if (h->desc.nn_mode != SMPC_NN_NONE) {
        if (h->net->nlayers == 0) return fail(h, SMPC_ESTATE, "nn_mode != NONE but smpc_set_mlp was not called");
        const int terminal = h->desc.nn_mode == SMPC_NN_TERMINAL;
        const int M = terminal ? B : B * N;          // the list's capacity
        int rc;
        if ((rc = ensure_nn_idx(h, (size_t)M))) return rc;
        const double* xn = x;
        if (dx && alpha) {
            hipLaunchKernelGGL(k_sqp_trial_states, dim3((unsigned)((nodes * 2 * NQ + 63) / 64)), dim3(64), 0, s, B, (N + 1) * 2 * NQ, x, dx,
                               alpha, mask, w.xt);
            xn = w.xt;
        }
        hipLaunchKernelGGL(k_sqp_nn_list, dim3((unsigned)((nodes + 63) / 64)), dim3(64), 0, s, B, N, terminal, p, mask, h->d_nn_idx.p, w.pos,
                           h->d_nn_cnt);
        HIPCHK(h, hipGetLastError());
        if ((rc = run_mlp<NQ>(h, M, 3, N, xn, false, rows_of_nodes(N + 1)))) return rc;
        y = h->d_y.p;
    }
    with_scene(h, B, [&](auto SCENE, auto sc) {
        return with_model(h, B, [&](auto MODEL, auto... md) {
            return with_row_bounds(h, B, [&](auto... rb) {
                hipLaunchKernelGGL((k_merit<NQ, SCENE, MODEL>), dim3(B), dim3(64), 0, s, h->d_desc, B, N, x0, x, u, p, dx, du, alpha, mask, y,
                                   w.pos, out, sc, md..., rb...);
                return SMPC_OK;
            });
        });
    });
    HIPCHK(h, hipGetLastError());
    if (y) HIPCHK(h, hipMemsetAsync(h->d_nn_cnt, 0, sizeof(int32_t), s));
    return SMPC_OK;
}

// The bounds smpc_check_guess tests against (h->gchk, a block of its own: the policy entry points keep h->chk warm with another
// layout): [x_min | x_max | tau_min | tau_max | row_lb | row_ub]
struct GchkBlock { double *x_min, *x_max, *tau_min, *tau_max, *row_lb, *row_ub; size_t doubles; };
GchkBlock gchk_block(double* base, int nq) {
    Carve m = dense(base);
    GchkBlock b{};
    b.x_min = m.take<double>(2 * nq);
    b.x_max = m.take<double>(2 * nq);
    b.tau_min = m.take<double>(nq);
    b.tau_max = m.take<double>(nq);
    b.row_lb = m.take<double>(SMPC_MAX_ROWS);
    b.row_ub = m.take<double>(SMPC_MAX_ROWS);
    b.doubles = m.off / sizeof(double);
    return b;
}
int upload_guess_bounds(smpc_handle* h, const smpc_guess_check* par) {
    const int nq = h->desc.nq, nr = h->desc.n_rows;
    std::vector<double> img(gchk_block(nullptr, nq).doubles, 0.0);
    const GchkBlock b = gchk_block(img.data(), nq);
    put(b.x_min, par->x_min, 2 * nq);
    put(b.x_max, par->x_max, 2 * nq);
    put(b.tau_min, par->tau_min, nq);
    put(b.tau_max, par->tau_max, nq);
    put(b.row_lb, par->row_lb_chk, nr);
    put(b.row_ub, par->row_ub_chk, nr);
    return h->gchk.upload(h, img);
}

// flags / worst of the instances whose mask byte is set: the forward-only network pass on their safe-set node (listed by
// k_guess_nn_list, so that masked-out instances cost no network rows), then k_check_guess.  The list's counter goes back to zero
// behind the chain (see d_nn_cnt).
template <int NQ>
int launch_check_guess(smpc_handle* h, int B, const double* x, const double* u, const smpc_guess_check* par, const uint8_t* mask,
                       int32_t* flags, double* worst) {
    const int N = h->N;
    hipStream_t s = h->stream;
    int rc;
    const float* y = nullptr;
    if (par->safe_node >= 0) {
        if ((rc = h->d_guess.reserve(h, "guess check scratch", sizeof(int32_t) * (size_t)B)) || (rc = ensure_nn_idx(h, (size_t)B))) return rc;
        hipLaunchKernelGGL(k_guess_nn_list, dim3((B + 63) / 64), dim3(64), 0, s, B, N, (int)par->safe_node, mask, h->d_nn_idx.p, h->d_guess.p,
                           h->d_nn_cnt);
        HIPCHK(h, hipGetLastError());
        if ((rc = run_mlp<NQ>(h, B, 3, N, x, false, rows_of_nodes(N + 1)))) return rc;
        y = h->d_y.p;
    }
    const GchkBlock c = gchk_block(h->gchk.d.p, NQ);
    with_scene(h, B, [&](auto SCENE, auto sc) {
        return with_model(h, B, [&](auto MODEL, auto... md) {
            hipLaunchKernelGGL((k_check_guess<NQ, SCENE, MODEL>), dim3(B), dim3(64), 0, s, h->d_desc, B, N, x, u, par->tol_x, par->tol_tau,
                               par->tol_dyn, par->tol_safe, par->alpha, (int)par->collision_first_node, (int)par->safe_node, c.x_min, c.x_max,
                               c.tau_min, c.tau_max, c.row_lb, c.row_ub, mask, y, (const int32_t*)h->d_guess.p, flags, worst, sc, md...);
            return SMPC_OK;
        });
    });
    HIPCHK(h, hipGetLastError());
    if (y) HIPCHK(h, hipMemsetAsync(h->d_nn_cnt, 0, sizeof(int32_t), s));
    return SMPC_OK;
}

// The small host arrays of smpc_ik_batch (h->ikb): [q_lo | q_hi | row_lb | row_ub], the joint arrays SMPC_MAX_NQ long whatever nq
struct IkbBlock { double *q_lo, *q_hi, *row_lb, *row_ub; size_t doubles; };
IkbBlock ikb_block(double* base) {
    Carve m = dense(base);
    IkbBlock b{};
    b.q_lo = m.take<double>(SMPC_MAX_NQ);
    b.q_hi = m.take<double>(SMPC_MAX_NQ);
    b.row_lb = m.take<double>(SMPC_MAX_ROWS);
    b.row_ub = m.take<double>(SMPC_MAX_ROWS);
    b.doubles = m.off / sizeof(double);
    return b;
}
int upload_ik_bounds(smpc_handle* h, const smpc_ik_params* par) {
    const int nq = h->desc.nq, nr = h->desc.n_rows;
    std::vector<double> img(ikb_block(nullptr).doubles, 0.0);
    const IkbBlock b = ikb_block(img.data());
    put(b.q_lo, par->q_lo, nq);
    put(b.q_hi, par->q_hi, nq);
    put(b.row_lb, par->row_lb, nr);
    put(b.row_ub, par->row_ub, nr);
    return h->ikb.upload(h, img);
}

// k_ik: one wavefront per instance, lane s = start s
template <int NQ>
int launch_ik(smpc_handle* h, int B, int S, const double* target, const double* q_start, const smpc_ik_params* par, const uint8_t* mask,
              double* q_out, int32_t* info, double* resid) {
    hipStream_t s = h->stream;
    const IkbBlock c = ikb_block(h->ikb.d.p);
    with_scene(h, B, [&](auto SCENE, auto sc) {
        hipLaunchKernelGGL((k_ik<NQ, SCENE>), dim3(B), dim3(64), 0, s, h->d_desc, B, S, target, q_start, (int)par->max_iter, par->tol_ee,
                           par->push, par->damping, par->damping_accept, par->damping_reject, par->damping_min, par->damping_max, c.q_lo,
                           c.q_hi, c.row_lb, c.row_ub, mask, q_out, info, resid, sc);
        return SMPC_OK;
    });
    HIPCHK(h, hipGetLastError());
    return SMPC_OK;
}

// The small host arrays of smpc_score_rollout (h->schk): [x_min | x_max | row_lb | row_ub | ee_ref]
struct SchkBlock { double *x_min, *x_max, *row_lb, *row_ub, *ee_ref; size_t doubles; };
SchkBlock schk_block(double* base, int nq) {
    Carve m = dense(base);
    SchkBlock b{};
    b.x_min = m.take<double>(2 * nq);
    b.x_max = m.take<double>(2 * nq);
    b.row_lb = m.take<double>(SMPC_MAX_ROWS);
    b.row_ub = m.take<double>(SMPC_MAX_ROWS);
    b.ee_ref = m.take<double>(3);
    b.doubles = m.off / sizeof(double);
    return b;
}
int upload_score_bounds(smpc_handle* h, const smpc_score_params* par) {
    const int nq = h->desc.nq, nr = h->desc.n_rows;
    std::vector<double> img(schk_block(nullptr, nq).doubles, 0.0);
    const SchkBlock b = schk_block(img.data(), nq);
    put(b.x_min, par->x_min, 2 * nq);
    put(b.x_max, par->x_max, 2 * nq);
    put(b.row_lb, par->row_lb_chk, nr);
    put(b.row_ub, par->row_ub_chk, nr);
    // (a call with traj does not read ee_ref: the block keeps the last one, so that alternating calls do not count as a change)
    // (nor does a call against the handle's curves, which gives neither)
    if (!par->traj && par->ee_ref) put(b.ee_ref, par->ee_ref, 3);
    else if (h->schk.cache.size() == img.size()) put(b.ee_ref, schk_block(h->schk.cache.data(), nq).ee_ref, 3);
    return h->schk.upload(h, img);
}

// scratch of smpc_score_rollout: the partials of every (segment, instance) and the running safe-set minimum of every instance
struct ScoreScratch {
    double* pd;         // [n_seg][SCORE_PD][B]
    int32_t* pi;        // [n_seg][SCORE_PI][B]
    double* gmin;       // [B]
    int32_t* gstep;     // [B]
    size_t bytes;
};
ScoreScratch score_layout(char* base, int B, int n_seg) {
    Carve m{base};
    ScoreScratch w{};
    w.pd = m.take<double>((size_t)n_seg * SCORE_PD * B);
    w.pi = m.take<int32_t>((size_t)n_seg * SCORE_PI * B);
    w.gmin = m.take<double>(B);
    w.gstep = m.take<int32_t>(B);
    w.bytes = m.off;
    return w;
}

// The network's forward pass reads the state log as flat rows in passes of at most this many rows, so that its buffers are those of
// one pass whatever n_steps * B is: 1 MiB of outputs with the one-kernel passes (256 wide, three hidden layers: ensure_mlp level 0),
// 2.1 GiB with the layer-by-layer chain (any other network: level 2, 2129 floats a row at H = 256)
constexpr long SCORE_MLP_ROWS = 1L << 18;

// out / outi of the instances whose mask byte is set: k_score_seg over (64 instances) x (segment), the network in bounded passes
// each followed by k_score_safe when the safe-set score is wanted, then k_score_combine
template <int NQ>
int launch_score(smpc_handle* h, int B, int n_steps, const double* x_log, const double* u_log, const int64_t* last_x,
                 const int64_t* last_u, const smpc_score_params* par, const double* traj, long traj_len, long traj_stride,
                 const uint8_t* mask, double* out, int32_t* outi) {
    constexpr int nx = 2 * NQ;
    hipStream_t s = h->stream;
    const int n_seg = n_steps / SCORE_SEG + 1;          // segments of the n_steps + 1 states
    int rc;
    if ((rc = h->d_score.reserve(h, "score scratch", score_layout(nullptr, B, n_seg).bytes))) return rc;
    const ScoreScratch w = score_layout(h->d_score.p, B, n_seg);
    const SchkBlock c = schk_block(h->schk.d.p, NQ);
    const unsigned gb = (unsigned)((B + 63) / 64);
    with_scene(h, B, [&](auto SCENE, auto sc) {
        hipLaunchKernelGGL((k_score_seg<NQ, SCENE>), dim3(gb, (unsigned)n_seg), dim3(64), 0, s, h->d_desc, B, n_steps, x_log, u_log, last_x,
                           last_u, c.x_min, c.x_max, c.row_lb, c.row_ub, c.ee_ref, traj, traj_len, traj_stride, mask, w.pd, w.pi, sc);
        return SMPC_OK;
    }, 0, false);      // (a log starts at time 0: state j in column col(j), whatever the clock says)
    HIPCHK(h, hipGetLastError());
    if (par->want_safe) {
        const long total = (long)(n_steps + 1) * B;
        for (long m0 = 0; m0 < total; m0 += SCORE_MLP_ROWS) {
            const long rows = total - m0 < SCORE_MLP_ROWS ? total - m0 : SCORE_MLP_ROWS;
            if ((rc = run_mlp<NQ>(h, (int)rows, 0, 0, x_log + m0 * nx, false, rows_step_major(B, m0)))) return rc;
            hipLaunchKernelGGL((k_score_safe<NQ>), dim3(gb), dim3(64), 0, s, h->d_desc, B, n_steps, m0, rows, m0 == 0 ? 1 : 0, x_log, last_x,
                               last_u, par->alpha, mask, (const float*)h->d_y.p, w.gmin, w.gstep);
            HIPCHK(h, hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_score_combine, dim3(gb), dim3(64), 0, s, B, n_steps, h->desc.Q, h->desc.R, last_x, last_u, mask,
                       (const double*)w.pd, (const int32_t*)w.pi, par->want_safe ? (const double*)w.gmin : (const double*)nullptr,
                       (const int32_t*)w.gstep, out, outi);
    HIPCHK(h, hipGetLastError());
    return SMPC_OK;
}

// ---- the streams of handles and rollout workers ----------------------------------------------------------------------------------
// SMPC_STREAM_PRIORITY (read once per process): 0 `default` = hipStreamCreateWithFlags as before this function existed, 1 `high` (what
// an unset variable means), 2 `low`; -1 = anything else, which smpc_create refuses.
int stream_route() {
    static const int v = [] {
        const char* e = getenv("SMPC_STREAM_PRIORITY");
        if (!e || !strcmp(e, "high")) return 1;
        return !strcmp(e, "default") ? 0 : (!strcmp(e, "low") ? 2 : -1);
    }();
    return v;
}

// The one place that makes an engine stream (smpc_create; the rollout workers are handles).  The runtime keeps a pool of hardware
// queues PER PRIORITY LEVEL, at most GPU_MAX_HW_QUEUES each (4 unless the process sets it), and gives a new stream the queue of its
// level's pool with the fewest users once the pool is full; two streams on one queue run in order.  At the default level the engine
// shares that pool with the null stream, torch's stream pool, RCCL and the runtime's own queues, and the third sub-batch of a bench
// process landed on a queue that already carried another (point 4b).  So every engine stream of the process is
// made at ONE level that nothing else in the process uses (the highest unless SMPC_STREAM_PRIORITY says otherwise; the handles stay
// equals, only the pool changes).  Where it stops helping: handles beyond the pool's size share queues as before -- the fifth live
// handle of a process with four queues per level (C3's five horizon groups beside the probe handle) takes turns with another.
// A device with one level, or a runtime that refuses the call as invalid / unsupported, gets the plain call; any other error is the
// caller's to report.
hipError_t create_handle_stream(int device, hipStream_t* s) {
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return e;
    const int route = stream_route();
    if (route > 0) {
        int least = 0, greatest = 0;     // (numerically: greatest priority <= least priority)
        e = hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (e == hipSuccess && least != greatest) e = hipStreamCreateWithPriority(s, hipStreamNonBlocking, route == 1 ? greatest : least);
        else if (e == hipSuccess) e = hipErrorNotSupported;
        if (e != hipErrorInvalidValue && e != hipErrorNotSupported) return e;
        (void)hipGetLastError();
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

}  // namespace

extern "C" {

int smpc_abi_version(void) { return SMPC_ABI_VERSION; }

const char* smpc_last_error(const smpc_handle* h) { return h ? h->err : g_create_err; }

int smpc_create(const smpc_problem_desc* desc, int device, smpc_handle** out) {
    if (!desc || !out) return fail(nullptr, SMPC_EINVAL, "null argument");
    *out = nullptr;
    if (stream_route() < 0)
        return fail(nullptr, SMPC_EINVAL, "SMPC_STREAM_PRIORITY=%s: expected default, high or low", getenv("SMPC_STREAM_PRIORITY"));
    if (desc->abi_version != SMPC_ABI_VERSION)
        return fail(nullptr, SMPC_EINVAL, "descriptor ABI %d, library ABI %d", desc->abi_version, SMPC_ABI_VERSION);
    if (desc->nq < 5 || desc->nq > SMPC_MAX_NQ) return fail(nullptr, SMPC_EINVAL, "nq=%d unsupported", desc->nq);
    if (desc->N < 1 || desc->N > SMPC_MAX_N) return fail(nullptr, SMPC_EINVAL, "N=%d outside 1..%d", desc->N, SMPC_MAX_N);
    if (desc->n_rows < 0 || desc->n_rows > SMPC_MAX_ROWS || desc->n_points < 1 || desc->n_points > SMPC_MAX_POINTS)
        return fail(nullptr, SMPC_EINVAL, "n_rows / n_points out of range");
    for (int i = 0; i < desc->n_points; i++)
        if (desc->points[i].link >= desc->nq) return fail(nullptr, SMPC_EINVAL, "point %d rides on link %d >= nq", i, desc->points[i].link);
    for (int r = 0; r < desc->n_rows; r++) {
        const smpc_row& row = desc->rows[r];
        if (row.kind < 0 || row.kind > SMPC_ROW_COORD || row.pa < 0 || row.pa >= desc->n_points)
            return fail(nullptr, SMPC_EINVAL, "row %d malformed", r);
    }
    // k_qp_ipm gives every two-sided constraint row (x box, torque, collision, safe-set) its own lane of a half-wavefront
    if (3 * desc->nq + desc->n_rows + 1 > 32)
        return fail(nullptr, SMPC_EINVAL, "3*nq + n_rows + 1 = %d constraint rows per stage exceed the 32 lanes of a half-wavefront",
                    3 * desc->nq + desc->n_rows + 1);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, SMPC_EHIP, "no HIP device visible: the engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(nullptr, SMPC_EINVAL, "device %d of %d", device, ndev);
    smpc_handle* h = new (std::nothrow) smpc_handle();
    if (!h) return fail(nullptr, SMPC_ENOMEM, "out of host memory");
    h->desc = *desc;
    h->device = device;
    h->N = desc->N;
    hipError_t e = create_handle_stream(device, &h->stream);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_desc, sizeof(smpc_problem_desc));
    if (e == hipSuccess) e = hipMemcpy(h->d_desc, desc, sizeof(smpc_problem_desc), hipMemcpyHostToDevice);
    for (int i = 0; i < 5 * smpc_handle::EV_RING && e == hipSuccess; i++) e = hipEventCreate(&h->ev_sets[i / 5][i % 5]);
    if (e != hipSuccess) {
        fail(nullptr, SMPC_EHIP, "device setup failed: %s", hipGetErrorString(e));
        smpc_destroy(h);
        return SMPC_EHIP;
    }
    int rc = upload_bounds(h, nullptr, nullptr);
    if (rc) {
        snprintf(g_create_err, sizeof(g_create_err), "%s", h->err);
        smpc_destroy(h);
        return rc;
    }
    *out = h;
    return SMPC_OK;
}

void smpc_destroy(smpc_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    for (smpc_handle* k : h->kids) smpc_destroy(k);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    for (auto& set : h->ev_sets) for (auto& e : set) if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->d_desc) (void)hipFree(h->d_desc);
    delete h;       // (and with it every buffer the handle owns)
}

int smpc_set_mlp(smpc_handle* h, int nlayers, const int32_t* dims, const float* const* W, const float* const* b,
                 int on_device) {
    if (!h || !dims || !W || !b) return fail(h, SMPC_EINVAL, "null argument");
    if (nlayers < 2 || nlayers > SMPC_MAX_LAYERS) return fail(h, SMPC_EINVAL, "nlayers=%d outside 2..%d", nlayers, SMPC_MAX_LAYERS);
    const int in = dims[0], H = dims[1];
    if (in != 2 * h->desc.nn_dof || in > MLP_KPAD) return fail(h, SMPC_EINVAL, "input width %d != 2*n_dof_safe_set", in);
    if (H % 64 != 0 || dims[nlayers] != 1) return fail(h, SMPC_EINVAL, "hidden width must be a multiple of 64 and output 1");
    for (int l = 1; l < nlayers; l++)
        if (dims[l] != H) return fail(h, SMPC_EINVAL, "hidden layers must share one width");
    (void)hipSetDevice(h->device);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (smpc_handle* k : h->kids) smpc_destroy(k);      // (workers read the weight block, which may move below)
    h->kids.clear();
    Net& net = h->own_net;
    net.nlayers = 0;    // (no network until every layer is in place)
    net.n_ctx = 0;      // (new weights mean no context: layer 0's context rows are rewritten as zeros below)
    h->ctx.clear();
    // one block for every layer's W^T (layer 0 padded to MLP_KPAD rows), W (layer 0 padded to MLP_NPAD columns) and b
    const auto layout = [&](char* base) {
        Carve m{base};
        for (int l = 0; l < nlayers; l++) {
            net.Wfwd[l] = m.take<float>((size_t)(l == 0 ? MLP_KPAD : dims[l]) * dims[l + 1]);
            net.Wbwd[l] = m.take<float>((size_t)dims[l + 1] * (l == 0 ? MLP_NPAD : dims[l]));
            net.bias[l] = m.take<float>(dims[l + 1]);
        }
        return m.off;
    };
    int rc;
    if ((rc = net.d_weights.reserve(h, "network weights", layout(nullptr)))) return rc;
    layout(net.d_weights.p);
    for (int l = 0; l < nlayers; l++) {
        const int ni = dims[l], no = dims[l + 1];
        std::vector<float> w((size_t)ni * no), bb(no);
        HIPCHK(h, hipMemcpy(w.data(), W[l], w.size() * sizeof(float), on_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
        HIPCHK(h, hipMemcpy(bb.data(), b[l], bb.size() * sizeof(float), on_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost));
        const int kf = l == 0 ? MLP_KPAD : ni;            // rows of the forward operand W^T
        const int nb = l == 0 ? MLP_NPAD : ni;            // columns of the backward operand W
        std::vector<float> wf((size_t)kf * no, 0.0f), wb((size_t)no * nb, 0.0f);
        for (int o = 0; o < no; o++)
            for (int i = 0; i < ni; i++) {
                wf[(size_t)i * no + o] = w[(size_t)o * ni + i];
                wb[(size_t)o * nb + i] = w[(size_t)o * ni + i];
            }
        HIPCHK(h, hipMemcpy(net.Wfwd[l], wf.data(), wf.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(net.Wbwd[l], wb.data(), wb.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(net.bias[l], bb.data(), bb.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    net.nlayers = nlayers;
    for (int l = 0; l <= nlayers; l++) net.dims[l] = dims[l];
    net.H = H;
    return SMPC_OK;
}

int smpc_set_mlp_activation(smpc_handle* h, int act) {
    if (!h) return SMPC_EINVAL;
    if (act < SMPC_ACT_GELU_TANH || act > SMPC_ACT_SILU) return fail(h, SMPC_EINVAL, "unknown activation %d", act);
    h->own_net.act = act;
    return SMPC_OK;
}

int smpc_set_mlp_context(smpc_handle* h, int n_ctx, const float* Wc, const double* ctx_mean, const double* ctx_std,
                         const double* ctx_default, int on_device) {
    if (!h) return SMPC_EINVAL;
    Net& net = h->own_net;
    if (net.nlayers == 0) return fail(h, SMPC_ESTATE, "smpc_set_mlp_context: smpc_set_mlp was not called");
    const int nd2 = 2 * h->desc.nn_dof, room = MLP_KPAD - nd2, H = net.dims[1];
    if (n_ctx < 0 || n_ctx > room)
        return fail(h, SMPC_EINVAL, "smpc_set_mlp_context: n_ctx=%d outside 0..%d: layer 0's input is padded to %d columns and the state "
                    "takes 2*n_dof_safe_set = %d of them", n_ctx, room, MLP_KPAD, nd2);
    const bool clear = n_ctx == 0 || !Wc;
    if (!clear && (!ctx_mean || !ctx_std || !ctx_default)) return fail(h, SMPC_EINVAL, "smpc_set_mlp_context: null argument");
    (void)hipSetDevice(h->device);
    std::vector<float> wc;
    double mean[MLP_KPAD] = {0}, std_[MLP_KPAD] = {0}, def[MLP_KPAD] = {0};
    if (!clear) {
        const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost;
        wc.resize((size_t)H * n_ctx);
        HIPCHK(h, hipMemcpy(wc.data(), Wc, wc.size() * sizeof(float), kind));
        HIPCHK(h, hipMemcpy(mean, ctx_mean, sizeof(double) * n_ctx, kind));
        HIPCHK(h, hipMemcpy(std_, ctx_std, sizeof(double) * n_ctx, kind));
        HIPCHK(h, hipMemcpy(def, ctx_default, sizeof(double) * n_ctx, kind));
        for (size_t i = 0; i < wc.size(); i++)
            if (!(wc[i] - wc[i] == 0.0f))
                return fail(h, SMPC_EINVAL, "smpc_set_mlp_context: Wc[%zu][%zu] is not finite", i / n_ctx, i % n_ctx);
        for (int c = 0; c < n_ctx; c++) {
            if (!(mean[c] - mean[c] == 0.0) || !(std_[c] - std_[c] == 0.0) || !(def[c] - def[c] == 0.0))
                return fail(h, SMPC_EINVAL, "smpc_set_mlp_context: ctx_mean / ctx_std / ctx_default of context number %d is not finite", c);
            if (!(std_[c] > 0.0)) return fail(h, SMPC_EINVAL, "smpc_set_mlp_context: ctx_std[%d] = %g: must be > 0", c, std_[c]);
        }
    }
    // rows 2 nn_dof .. MLP_KPAD - 1 of layer 0's forward operand W^T [MLP_KPAD][H]: the context columns, zero behind them.  The
    // backward operand keeps its zero columns: no derivative with respect to the context is formed.
    std::vector<float> rows((size_t)room * H, 0.0f);
    float defn[MLP_KPAD] = {0};
    if (!clear) {
        for (int o = 0; o < H; o++)
            for (int c = 0; c < n_ctx; c++) rows[(size_t)c * H + o] = wc[(size_t)o * n_ctx + c];
        for (int c = 0; c < n_ctx; c++) defn[c] = (float)((def[c] - mean[c]) / std_[c]);
    }
    int rc;
    if (!clear && (rc = net.d_default_ctx.reserve(h, "default context", sizeof(defn)))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (smpc_handle* k : h->kids) HIPCHK(h, hipStreamSynchronize(k->stream));      // (the workers read these weights too)
    net.n_ctx = 0;
    h->ctx.clear();     // (an instance context belongs to the context columns it was normalised for)
    if (room > 0) HIPCHK(h, hipMemcpy(net.Wfwd[0] + (size_t)nd2 * H, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
    if (clear) return SMPC_OK;
    HIPCHK(h, hipMemcpy(net.d_default_ctx.p, defn, sizeof(defn), hipMemcpyHostToDevice));
    for (int c = 0; c < MLP_KPAD; c++) { net.ctx_mean[c] = mean[c]; net.ctx_std[c] = c < n_ctx ? std_[c] : 1.0; }
    net.n_ctx = n_ctx;
    return SMPC_OK;
}

int smpc_set_instance_context_track(smpc_handle* h, int B, int64_t T, const double* ctx, int on_device) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    if (!ctx) { h->ctx.clear(); return SMPC_OK; }
    const Net& net = *h->net;
    if (net.n_ctx == 0)
        return fail(h, SMPC_EINVAL, "smpc_set_instance_context: the network has no context columns (smpc_set_mlp_context was not called)");
    if (B <= 0) return fail(h, SMPC_EINVAL, "bad batch size");
    if (T < 1 || T > INT32_MAX)
        return fail(h, SMPC_EINVAL, "smpc_set_instance_context_track: T=%lld: a track has at least one time column (and fewer than 2^31)",
                    (long long)T);
    const int nc = net.n_ctx;
    const size_t n = (size_t)B * (size_t)T * nc;
    std::vector<float> norm;
    if (!on_device) {
        // (device pointers are taken as they are: reading them back would synchronise)
        norm.resize(n);
        for (size_t i = 0; i < n; i++) {
            if (!(ctx[i] - ctx[i] == 0.0)) {
                const size_t bt = i / nc;
                if (T == 1) return fail(h, SMPC_EINVAL, "context of instance %zu (of B=%d), number %zu (of %d) is not finite", bt, B, i % nc, nc);
                return fail(h, SMPC_EINVAL, "context track of instance %zu (of B=%d), column %zu (of T=%lld), number %zu (of %d) is not finite",
                            bt / (size_t)T, B, bt % (size_t)T, (long long)T, i % nc, nc);
            }
            norm[i] = (float)((ctx[i] - net.ctx_mean[i % nc]) / net.ctx_std[i % nc]);
        }
    }
    int rc;
    if ((rc = h->ctx.room(h, n))) return rc;
    if (on_device) {
        CtxNorm nm;
        for (int c = 0; c < MLP_KPAD; c++) { nm.mean[c] = net.ctx_mean[c]; nm.std[c] = net.ctx_std[c]; }
        hipLaunchKernelGGL(k_ctx_normalise, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, (long)n, nc, ctx, nm, h->ctx.d.p);
        HIPCHK(h, hipGetLastError());
    } else if ((rc = h->ctx.upload(h, norm.data(), n, false)))
        return rc;
    h->ctx.commit(B);
    h->ctx_T = T;
    h->ctx_fc = false;      // (a context of the caller's replaces one that a forecast wrote: read by the clock again)
    return SMPC_OK;
}

int smpc_set_instance_context(smpc_handle* h, int B, const double* ctx, int on_device) {
    return smpc_set_instance_context_track(h, B, 1, ctx, on_device);
}

int smpc_set_qp_mode(smpc_handle* h, int mode) {
    if (!h) return SMPC_EINVAL;
    if (mode < SMPC_QP_AUTO || mode > SMPC_QP_LATENCY) return fail(h, SMPC_EINVAL, "qp mode %d (SMPC_QP_AUTO, _THROUGHPUT, _LATENCY)", mode);
    h->qp_mode = mode;
    return SMPC_OK;
}

int smpc_set_qp_crew(smpc_handle* h, double fraction, int waves) {
    if (!h) return SMPC_EINVAL;
    if (waves < 0 || (waves == 0 && !(fraction > 0.0 && fraction <= 1.0)))
        return fail(h, SMPC_EINVAL, "qp crew: fraction %g outside (0, 1], or %d wavefronts", fraction, waves);
    h->qp_crew = waves > 0 ? -1.0 : fraction;
    h->qp_crew_waves = waves;
    return SMPC_OK;
}

int smpc_set_horizon(smpc_handle* h, int N) {
    if (!h) return SMPC_EINVAL;
    if (N < 1 || N > SMPC_MAX_N) return fail(h, SMPC_EINVAL, "N=%d outside 1..%d", N, SMPC_MAX_N);
    (void)hipSetDevice(h->device);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->N = N;
    h->bounds.clear();      // (the slots laid out by the horizon ...
    h->rowb.clear();
    drop_forecast(h);       //  ... and a forecast, N + 1 columns of it; the world it was made from stays)
    h->order_B = 0;
    // every buffer laid out by the horizon starts afresh (zeroed where that is its contract) in the next call that needs it
    for (DevBuf<double>* buf : {&h->d_zl, &h->bounds.d, &h->rowb.d, &h->d_ev, &h->d_nn, &h->d_ws, &h->d_hrec}) buf->release();
    h->d_par.release();
    h->d_sqp.release();
    h->d_guess.release();
    return upload_bounds(h, nullptr, nullptr);
}

int smpc_set_stage_bounds(smpc_handle* h, const double* lo, const double* hi) {
    if (!h) return SMPC_EINVAL;
    if ((lo == nullptr) != (hi == nullptr)) return fail(h, SMPC_EINVAL, "lo and hi must both be given or both be NULL");
    (void)hipSetDevice(h->device);
    return upload_bounds(h, lo, hi);
}

int smpc_set_slack_weights(smpc_handle* h, const double* zl) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!zl) {
        h->d_zl.release();
        return SMPC_OK;
    }
    for (int k = 1; k <= h->N; k++)
        if (!(zl[k] >= 0.0)) return fail(h, SMPC_EINVAL, "slack weight of node %d is negative or NaN", k);
    int rc;
    if ((rc = h->d_zl.reserve(h, "slack weights", sizeof(double) * (h->N + 1)))) return rc;
    HIPCHK(h, hipMemcpy(h->d_zl.p, zl, sizeof(double) * (h->N + 1), hipMemcpyHostToDevice));
    return SMPC_OK;
}

int smpc_set_instance_bounds(smpc_handle* h, int B, const double* lo, const double* hi, int on_device) {
    if (!h) return SMPC_EINVAL;
    if ((lo == nullptr) != (hi == nullptr)) return fail(h, SMPC_EINVAL, "lo and hi must both be given or both be NULL");
    (void)hipSetDevice(h->device);
    if (!lo) { h->bounds.clear(); return SMPC_OK; }
    if (B <= 0) return fail(h, SMPC_EINVAL, "bad batch size");
    const size_t n = (size_t)B * (h->N + 1) * 2 * h->desc.nq;
    int rc;
    if ((rc = ensure_instance_bounds(h, B, false)) || (rc = h->bounds.upload(h, lo, n, on_device != 0)) ||
        (rc = h->bounds.upload(h, hi, n, on_device != 0, instance_hi(h) - h->bounds.d.p)))
        return rc;
    h->bounds.commit(B);
    return SMPC_OK;
}

int smpc_set_instance_row_bounds(smpc_handle* h, int B, const double* lo, const double* hi, int on_device) {
    if (!h) return SMPC_EINVAL;
    if ((lo == nullptr) != (hi == nullptr))
        return fail(h, SMPC_EINVAL, "smpc_set_instance_row_bounds: lo and hi must both be given or both be NULL");
    (void)hipSetDevice(h->device);
    if (!lo) { h->rowb.clear(); return SMPC_OK; }
    if (B <= 0) return fail(h, SMPC_EINVAL, "bad batch size");
    const int nr = h->desc.n_rows;
    if (nr == 0) return fail(h, SMPC_EINVAL, "the problem has no collision rows: there are no row bounds to set");
    const size_t n = (size_t)B * (h->N + 1) * nr;
    if (!on_device) {
        // (device pointers are taken as they are: reading them back would synchronise)
        for (size_t i = 0; i < n; i++) {
            const int b = (int)(i / ((size_t)(h->N + 1) * nr)), k = (int)(i / nr % (h->N + 1)), r = (int)(i % nr);
            if (lo[i] != lo[i] || hi[i] != hi[i])
                return fail(h, SMPC_EINVAL, "row bounds of instance %d, node %d, row %d: NaN", b, k, r);
            if (fabs(lo[i]) < SMPC_INF && fabs(hi[i]) < SMPC_INF && lo[i] > hi[i])
                return fail(h, SMPC_EINVAL, "row bounds of instance %d, node %d, row %d: lo %g > hi %g", b, k, r, lo[i], hi[i]);
        }
    }
    // [lo | hi]: the same B finds both halves where they were, so a captured solve keeps seeing them
    int rc;
    if ((rc = h->rowb.room(h, 2 * n)) || (rc = h->rowb.upload(h, lo, n, on_device != 0)) || (rc = h->rowb.upload(h, hi, n, on_device != 0, n)))
        return rc;
    h->rowb.commit(B);
    return SMPC_OK;
}

// The one setter of a table of scene records [B][T][n_rows][SMPC_SCENE_ROW]: the scene slot (smpc_set_instance_scene_track) and the
// world (smpc_set_instance_world_track) share layout, validation and the slot rule.
static int set_scene_table(smpc_handle* h, InstSlot<double>& slot, int64_t& slot_T, const char* who, int B, int64_t T, const double* geom,
                           int on_device) {
    if (B <= 0) return fail(h, SMPC_EINVAL, "bad batch size");
    if (T < 1) return fail(h, SMPC_EINVAL, "%s: T=%lld: a track has at least one time column", who, (long long)T);
    const int nr = h->desc.n_rows;
    if (nr == 0) return fail(h, SMPC_EINVAL, "the problem has no collision rows: there is no scene to set");
    const size_t n = (size_t)B * (size_t)T * nr * SMPC_SCENE_ROW;
    if (!on_device) {
        // the fields a row's kind reads must be finite (device pointers are taken as they are: reading them back would synchronise)
        for (size_t bt = 0; bt < (size_t)B * (size_t)T; bt++)
            for (int r = 0; r < nr; r++) {
                const double* g = geom + (bt * nr + r) * SMPC_SCENE_ROW;
                const int kind = h->desc.rows[r].kind;
                const int lo = kind == SMPC_ROW_COORD ? 6 : 0;
                const int hi = kind == SMPC_ROW_SEG_FIXEDSEG ? 6 : (kind == SMPC_ROW_SEG_POINT || kind == SMPC_ROW_POINT_POINT ? 3 : (kind == SMPC_ROW_COORD ? 7 : 0));
                for (int i = lo; i < hi; i++)
                    if (!(g[i] - g[i] == 0.0)) {
                        if (T == 1) return fail(h, SMPC_EINVAL, "scene of instance %d, row %d (kind %d): entry %d is not finite", (int)bt, r, kind, i);
                        return fail(h, SMPC_EINVAL, "scene track of instance %d, column %lld, row %d (kind %d): entry %d is not finite",
                                    (int)(bt / (size_t)T), (long long)(bt % (size_t)T), r, kind, i);
                    }
            }
    }
    int rc;
    if ((rc = slot.room(h, n)) || (rc = slot.upload(h, geom, n, on_device != 0))) return rc;
    slot.commit(B);
    slot_T = T;
    return SMPC_OK;
}

int smpc_set_instance_scene_track(smpc_handle* h, int B, int64_t T, const double* geom, int on_device) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    if (!geom) { h->scene.clear(); h->scene_fc = false; return SMPC_OK; }
    const int rc = set_scene_table(h, h->scene, h->scene_T, "smpc_set_instance_scene_track", B, T, geom, on_device);
    if (rc) return rc;
    // a scene of the caller's replaces a forecast: the slot is read by the clock again, and a context that the forecast wrote goes
    // with it (a setter's own context stays)
    h->scene_fc = false;
    if (h->ctx_fc) { h->ctx.clear(); h->ctx_fc = false; }
    return SMPC_OK;
}

int smpc_set_instance_world_track(smpc_handle* h, int B, int64_t T, const double* geom, int on_device) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    if (!geom) {
        h->world.clear();
        h->seen.clear();        // (an observation without its world is stale ...
        drop_forecast(h);       //  ... and so is a forecast)
        return SMPC_OK;
    }
    return set_scene_table(h, h->world, h->world_T, "smpc_set_instance_world_track", B, T, geom, on_device);
}

int smpc_set_instance_observed_track(smpc_handle* h, int B, int64_t T, const double* geom, int on_device) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    if (!geom) { h->seen.clear(); return SMPC_OK; }
    return set_scene_table(h, h->seen, h->seen_T, "smpc_set_instance_observed_track", B, T, geom, on_device);
}

// What every entry point that reads S -- the three forecasts and smpc_forecast_row_margin -- asks of the world, of a fit's window and
// degree, and of the observed track, in this order, with the caller's name in the message.
static int check_forecast_world(smpc_handle* h, const char* who, int B) {
    if (!h->world.B) return fail(h, SMPC_ESTATE, "%s: no world is set (smpc_set_instance_world_track)", who);
    if (B != h->world.B)
        return fail(h, SMPC_EINVAL, "%s: batch size %d, but the instance world track was set for %d instances "
                    "(smpc_set_instance_world_track: clear it or set one of this size)", who, B, h->world.B);
    return SMPC_OK;
}
static int check_fit_shape(smpc_handle* h, const char* who, int window, int degree) {
    if (window < 1 || window > SMPC_FIT_MAX)
        return fail(h, SMPC_EINVAL, "%s: window %d: a fit takes 1 to SMPC_FIT_MAX = %d samples", who, window, SMPC_FIT_MAX);
    if (degree < 0 || degree > 2)
        return fail(h, SMPC_EINVAL, "%s: degree %d: a polynomial of degree 0, 1 or 2", who, degree);
    return SMPC_OK;
}
static int check_forecast_observed(smpc_handle* h, const char* who) {
    if (h->seen.B && (h->seen.B != h->world.B || h->seen_T != h->world_T))
        return fail(h, SMPC_EINVAL, "%s: the instance observed track was set for %d instances and %lld columns, but the instance world "
                    "track for %d instances and %lld columns (smpc_set_instance_observed_track: clear it or set one of the world's "
                    "shape)", who, h->seen.B, (long long)h->seen_T, h->world.B, (long long)h->world_T);
    return SMPC_OK;
}
// S as the fits read it: the observed track while one is set, else the world, at the scene clock (the window grows with the clock
// even where T = 1 leaves one column to read)
static SceneSrc fit_source(const smpc_handle* h) {
    return SceneSrc{h->seen.B ? h->seen.d.p : h->world.d.p, h->scene_clock, h->world_T, 0};
}

// The one body of smpc_forecast_scene (fit = false: `what` is its mode), smpc_forecast_scene_fit (fit = true: `what` is its window,
// degree 1) and smpc_forecast_scene_poly (fit = true with its degree); `who` names the entry point in every message.  S, "what was seen", is the observed track while one is set and the world
// otherwise; SMPC_FORECAST_TRUE reads the world whatever was observed.
// kal: smpc_forecast_scene_kalman's call (fit and what are not read then).  With advance it reads S as a fit does; without, it reads no
// table, so it needs no world and takes any B.
struct KalmanCall { KalmanArgs ka; double* state; bool advance; };
static int forecast_into_scene(smpc_handle* h, const char* who, int B, bool fit, int what, int n_sel, const int32_t* select,
                               int degree = 1, const KalmanCall* kal = nullptr) {
    const int mode = what, window = what;
    const bool reads_S = !kal || kal->advance;
    int rc;
    if (reads_S && (rc = check_forecast_world(h, who, B))) return rc;
    if (!reads_S && B <= 0) return fail(h, SMPC_EINVAL, "%s: bad batch size %d", who, B);
    if (!reads_S && h->desc.n_rows == 0) return fail(h, SMPC_EINVAL, "%s: the problem has no collision rows: there is no scene to forecast", who);
    if (!kal && !fit && mode != SMPC_FORECAST_HOLD && mode != SMPC_FORECAST_CV && mode != SMPC_FORECAST_TRUE)
        return fail(h, SMPC_EINVAL, "%s: mode %d (SMPC_FORECAST_HOLD, _CV, _TRUE)", who, mode);
    if (!kal && fit && (rc = check_fit_shape(h, who, window, degree))) return rc;
    if (reads_S && (rc = check_forecast_observed(h, who))) return rc;
    const Net& net = *h->net;
    const int nr = h->desc.n_rows, N = h->N, nc = net.n_ctx;
    if (n_sel < 0) return fail(h, SMPC_EINVAL, "%s: n_sel=%d", who, n_sel);
    ForecastSel sel{};
    CtxNorm nm{};
    if (n_sel > 0) {
        if (!select) return fail(h, SMPC_EINVAL, "%s: n_sel=%d with select == NULL", who, n_sel);
        if (nc == 0)
            return fail(h, SMPC_EINVAL, "%s: n_sel=%d, but the network has no context columns (smpc_set_mlp_context was not called)", who,
                        n_sel);
        if (n_sel != nc) return fail(h, SMPC_EINVAL, "%s: n_sel=%d, but the network has n_ctx=%d context columns", who, n_sel, nc);
        for (int i = 0; i < n_sel; i++) {
            const int r = select[2 * i], s = select[2 * i + 1];
            if (r < 0 || r >= nr || s < 0 || s >= SMPC_SCENE_ROW)
                return fail(h, SMPC_EINVAL, "%s: select[%d] = (row %d, slot %d) outside %d rows x %d slots", who, i, r, s, nr, SMPC_SCENE_ROW);
            sel.row[i] = r;
            sel.slot[i] = s;
        }
        for (int c = 0; c < MLP_KPAD; c++) { nm.mean[c] = net.ctx_mean[c]; nm.std[c] = net.ctx_std[c]; }
    }
    // room first, launches last: a call refused for growth under capture has changed nothing.  A buffer that did grow lost its old
    // content with its old allocation, so the slot is empty until the commit below.
    const size_t n = (size_t)B * (N + 1) * nr * SMPC_SCENE_ROW, n_ctx_el = (size_t)B * (N + 1) * n_sel;
    const bool scene_grows = n * sizeof(double) > h->scene.d.cap, ctx_grows = n_ctx_el * sizeof(float) > h->ctx.d.cap;
    if ((scene_grows || ctx_grows) && capturing(h))
        return fail(h, SMPC_ESTATE, "%s: the %s must grow to %zu bytes while the stream is being captured: run one eager call of this size "
                    "first", who, scene_grows ? h->scene.noun : h->ctx.noun, scene_grows ? n * sizeof(double) : n_ctx_el * sizeof(float));
    if (scene_grows) h->scene.clear();
    if ((rc = h->scene.room(h, n))) return rc;
    if (ctx_grows) h->ctx.clear();
    if (n_sel > 0 && (rc = h->ctx.room(h, n_ctx_el))) return rc;
    const SceneSrc world{h->world.d.p, h->world_T > 1 ? h->scene_clock : nullptr, h->world_T, 0};
    SceneSrc seen = world;      // (its (B, T) are the world's: checked above)
    if (h->seen.B) seen.geom = h->seen.d.p;
    if (fit) seen.clock = h->scene_clock;       // (the fit's window grows with the clock even where T = 1 leaves one column to read)
    const int n_rec = B * nr;
    // (one-wavefront blocks, as for every small kernel of the policy step: see check_nodes_dev)
    const dim3 grd((unsigned)((n_rec + 63) / 64)), blk(64);
    // (the fit and the polynomial last: a kernel's place in the code object follows its first mention, and the older ones keep theirs)
    if (!kal && !fit && mode == SMPC_FORECAST_HOLD)
        hipLaunchKernelGGL((k_scene_forecast<SMPC_FORECAST_HOLD>), grd, blk, 0, h->stream, n_rec, nr, N, seen, h->scene.d.p);
    else if (!kal && !fit && mode == SMPC_FORECAST_CV)
        hipLaunchKernelGGL((k_scene_forecast<SMPC_FORECAST_CV>), grd, blk, 0, h->stream, n_rec, nr, N, seen, h->scene.d.p);
    else if (!kal && !fit)
        hipLaunchKernelGGL((k_scene_forecast<SMPC_FORECAST_TRUE>), grd, blk, 0, h->stream, n_rec, nr, N, world, h->scene.d.p);
    else if (!kal && degree == 1)       // four lanes to a record: see k_scene_fit
        hipLaunchKernelGGL(k_scene_fit, dim3((unsigned)((4 * (size_t)n_rec + 63) / 64)), blk, 0, h->stream, 4 * n_rec, nr, N, window, seen,
                           h->scene.d.p);
    else if (!kal)                      // degrees 0 and 2: the same mapping
        hipLaunchKernelGGL(k_scene_poly, dim3((unsigned)((4 * (size_t)n_rec + 63) / 64)), blk, 0, h->stream, 4 * n_rec, nr, N, window, degree,
                           seen, h->scene.d.p);
    else {                              // the filter: the same mapping again; the row kinds travel by value
        KalmanKinds kinds{};
        for (int r = 0; r < nr; r++) kinds.kind[r] = h->desc.rows[r].kind;
        const dim3 grd4((unsigned)((4 * (size_t)n_rec + 63) / 64));
        seen.clock = h->scene_clock;    // (the filter advances with the clock even where T = 1 leaves one column to read)
        if (kal->advance)
            hipLaunchKernelGGL((k_scene_kalman<true>), grd4, blk, 0, h->stream, 4 * n_rec, nr, N, kal->ka, kinds, seen, kal->state, h->scene.d.p);
        else
            hipLaunchKernelGGL((k_scene_kalman<false>), grd4, blk, 0, h->stream, 4 * n_rec, nr, N, kal->ka, kinds, SceneSrc{}, kal->state,
                               h->scene.d.p);
    }
    HIPCHK(h, hipGetLastError());
    h->scene.commit(B);
    h->scene_T = N + 1;
    h->scene_fc = true;
    if (n_sel > 0) {
        hipLaunchKernelGGL(k_forecast_context, dim3((unsigned)((n_ctx_el + 63) / 64)), blk, 0, h->stream, (long)n_ctx_el, nc, nr,
                           h->scene.d.p, sel, nm, h->ctx.d.p);
        HIPCHK(h, hipGetLastError());
        h->ctx.commit(B);
        h->ctx_T = N + 1;
        h->ctx_fc = true;
    }
    return SMPC_OK;
}

int smpc_forecast_scene(smpc_handle* h, int B, int mode, int n_sel, const int32_t* select) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    return forecast_into_scene(h, "smpc_forecast_scene", B, false, mode, n_sel, select);
}

int smpc_forecast_scene_fit(smpc_handle* h, int B, int window, int n_sel, const int32_t* select) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    return forecast_into_scene(h, "smpc_forecast_scene_fit", B, true, window, n_sel, select);
}

int smpc_forecast_scene_poly(smpc_handle* h, int B, int window, int degree, int n_sel, const int32_t* select) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    return forecast_into_scene(h, "smpc_forecast_scene_poly", B, true, window, n_sel, select, degree);
}

// What the two margin entry points (smpc_forecast_row_margin, smpc_kalman_row_margin) share: the descriptor's rows by value with the
// crossing-sides check, and the slot's room for [lo | hi] of n doubles each.
static int margin_rows(smpc_handle* h, const char* who, double d_max, MarginRows* rows) {
    for (int r = 0; r < h->desc.n_rows; r++) {
        const smpc_row& R = h->desc.rows[r];
        if (R.kind == SMPC_ROW_COORD && fabs(R.lb) < SMPC_INF && fabs(R.ub) < SMPC_INF && R.lb + d_max > R.ub - d_max)
            return fail(h, SMPC_EINVAL, "%s: row %d: d_max=%g makes its sides cross (%g > %g)", who, r, d_max, R.lb + d_max, R.ub - d_max);
        rows->kind[r] = R.kind;
        rows->lb[r] = R.lb;
        rows->ub[r] = R.ub;
        // (on the host: the very double problem.inflated_row_bounds squares; read only where the row is a squared distance with a lower side)
        rows->sqrt_lb[r] = R.kind != SMPC_ROW_COORD && R.lb >= 0.0 ? sqrt(R.lb) : 0.0;
    }
    return SMPC_OK;
}
static int rowb_room_for_margin(smpc_handle* h, const char* who, size_t n) {
    // room first, launch last: a call refused for growth under capture has changed nothing; a buffer that did grow lost its old
    // content, so the slot is empty until the commit
    const bool grows = 2 * n * sizeof(double) > h->rowb.d.cap;
    if (grows && capturing(h))
        return fail(h, SMPC_ESTATE, "%s: the %s must grow to %zu bytes while the stream is being captured: run one eager call of this size "
                    "first", who, h->rowb.noun, 2 * n * sizeof(double));
    if (grows) h->rowb.clear();
    return h->rowb.room(h, 2 * n);
}

// The row-bounds slot filled from what was seen: the margins of k_fit_margin as the table that
// smpc_set_instance_row_bounds takes.  Reads S and the clock as smpc_forecast_scene_poly does; neither needs nor touches the scene slot.
int smpc_forecast_row_margin(smpc_handle* h, int B, int window, int degree, double z, double sigma_prior, double base_a, double base_b,
                             double d_max) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    const char* who = "smpc_forecast_row_margin";
    const int nr = h->desc.n_rows, N = h->N;
    // (first: a descriptor without rows takes no world either)
    if (nr == 0) return fail(h, SMPC_EINVAL, "%s: the problem has no collision rows: there are no row bounds to set", who);
    int rc;
    if ((rc = check_forecast_world(h, who, B)) || (rc = check_fit_shape(h, who, window, degree)) || (rc = check_forecast_observed(h, who)))
        return rc;
    const struct { const char* name; double v; } args[] = {{"z", z}, {"sigma_prior", sigma_prior}, {"base_a", base_a}, {"base_b", base_b},
                                                           {"d_max", d_max}};
    for (const auto& a : args)
        if (!(a.v >= 0.0 && a.v - a.v == 0.0))
            return fail(h, SMPC_EINVAL, "%s: %s=%g: a finite number that is not negative", who, a.name, a.v);
    MarginRows rows{};
    if ((rc = margin_rows(h, who, d_max, &rows))) return rc;
    const size_t n = (size_t)B * (N + 1) * nr;
    if ((rc = rowb_room_for_margin(h, who, n))) return rc;
    const int n_piece = 4 * B * nr;     // four lanes to a record: see k_fit_margin
    const MarginArgs ma{z, sigma_prior * sigma_prior, base_a, base_b, d_max};
    hipLaunchKernelGGL(k_fit_margin, dim3((unsigned)(((size_t)n_piece + 63) / 64)), dim3(64), 0, h->stream, n_piece, nr, N, window, degree,
                       fit_source(h), ma, rows, h->rowb.d.p, h->rowb.d.p + n);
    HIPCHK(h, hipGetLastError());
    h->rowb.commit(B);
    return SMPC_OK;
}

// What both filter entry points ask of the model, naming the argument; ka: the model as the kernels take it (problem.kalman_noise)
static int check_kalman(smpc_handle* h, const char* who, const smpc_kalman_params* par, const double* state, KalmanArgs* ka) {
    if (!par) return fail(h, SMPC_EINVAL, "%s: par == NULL", who);
    if (!state) return fail(h, SMPC_EINVAL, "%s: state == NULL", who);
    if (par->degree < 0 || par->degree > 2) return fail(h, SMPC_EINVAL, "%s: degree %d: a model of degree 0, 1 or 2", who, par->degree);
    if (!(par->r > 0.0 && par->r - par->r == 0.0)) return fail(h, SMPC_EINVAL, "%s: r=%g: a finite number above zero", who, par->r);
    const struct { const char* name; double v; } args[] = {{"q", par->q}, {"v0", par->v0}, {"a0", par->a0}};
    for (const auto& a : args)
        if (!(a.v >= 0.0 && a.v - a.v == 0.0))
            return fail(h, SMPC_EINVAL, "%s: %s=%g: a finite number that is not negative", who, a.name, a.v);
    if (!(par->beta >= 0.0 && par->beta <= 1.0)) return fail(h, SMPC_EINVAL, "%s: beta=%g: a number in [0, 1]", who, par->beta);
    const int p = par->degree;
    // (volatile: every product is one rounded multiplication, whatever the host compiler would like to fold or fuse)
    volatile double gq[3] = {0.0, 0.0, 0.0};
    if (p == 0) gq[0] = par->q;
    if (p == 1) { gq[0] = par->q * 0.5; gq[1] = par->q; }
    if (p == 2) { gq[0] = par->q * (1.0 / 6.0); gq[1] = par->q * 0.5; gq[2] = par->q; }
    *ka = KalmanArgs{p, 0, gq[0] * gq[0], gq[0] * gq[1], gq[0] * gq[2], gq[1] * gq[1], gq[1] * gq[2], gq[2] * gq[2],
                     par->r * par->r, par->v0 * par->v0, par->a0 * par->a0, par->beta};
    return SMPC_OK;
}

int smpc_forecast_scene_kalman(smpc_handle* h, int B, const smpc_kalman_params* par, double* state, int advance, int n_sel,
                               const int32_t* select) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    const char* who = "smpc_forecast_scene_kalman";
    KalmanCall kal{{}, state, advance != 0};
    int rc;
    if ((rc = check_kalman(h, who, par, state, &kal.ka))) return rc;
    return forecast_into_scene(h, who, B, false, 0, n_sel, select, 1, &kal);
}

// The row-bounds slot filled from the filter's covariance: k_kalman_margin's margins as the table that
// smpc_set_instance_row_bounds takes.  Reads the state alone: no world, no clock, not the scene slot.
int smpc_kalman_row_margin(smpc_handle* h, int B, const smpc_kalman_params* par, const double* state, double z, double base_a,
                           double base_b, double d_max) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    const char* who = "smpc_kalman_row_margin";
    const int nr = h->desc.n_rows, N = h->N;
    if (nr == 0) return fail(h, SMPC_EINVAL, "%s: the problem has no collision rows: there are no row bounds to set", who);
    if (B <= 0) return fail(h, SMPC_EINVAL, "%s: bad batch size %d", who, B);
    KalmanArgs ka{};
    int rc;
    if ((rc = check_kalman(h, who, par, state, &ka))) return rc;
    const struct { const char* name; double v; } args[] = {{"z", z}, {"base_a", base_a}, {"base_b", base_b}, {"d_max", d_max}};
    for (const auto& a : args)
        if (!(a.v >= 0.0 && a.v - a.v == 0.0))
            return fail(h, SMPC_EINVAL, "%s: %s=%g: a finite number that is not negative", who, a.name, a.v);
    MarginRows rows{};
    if ((rc = margin_rows(h, who, d_max, &rows))) return rc;
    const size_t n = (size_t)B * (N + 1) * nr;
    if ((rc = rowb_room_for_margin(h, who, n))) return rc;
    const int n_rec = B * nr;       // a thread to a record: see k_kalman_margin
    const MarginArgs ma{z, 0.0, base_a, base_b, d_max};
    hipLaunchKernelGGL(k_kalman_margin, dim3((unsigned)(((size_t)n_rec + 63) / 64)), dim3(64), 0, h->stream, n_rec, nr, N, ka, ma, rows, state,
                       h->rowb.d.p, h->rowb.d.p + n);
    HIPCHK(h, hipGetLastError());
    h->rowb.commit(B);
    return SMPC_OK;
}

int smpc_get_instance_row_bounds(smpc_handle* h, int B, double* lo, double* hi, int on_device) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    const char* who = "smpc_get_instance_row_bounds";
    if (!lo || !hi) return fail(h, SMPC_EINVAL, "%s: lo and hi must both be given", who);
    if (!h->rowb.B) return fail(h, SMPC_ESTATE, "%s: no %s is set (%s, smpc_forecast_row_margin)", who, h->rowb.noun, h->rowb.setter);
    int rc;
    if ((rc = h->rowb.guard(h, B, who))) return rc;
    const size_t n = (size_t)B * (h->N + 1) * h->desc.n_rows;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(h, hipMemcpyAsync(lo, h->rowb.d.p, n * sizeof(double), kind, h->stream));
    HIPCHK(h, hipMemcpyAsync(hi, h->rowb.d.p + n, n * sizeof(double), kind, h->stream));
    if (!on_device) HIPCHK(h, hipStreamSynchronize(h->stream));
    return SMPC_OK;
}

// a scene that stands still: the track of one column
int smpc_set_instance_scene(smpc_handle* h, int B, const double* geom, int on_device) {
    return smpc_set_instance_scene_track(h, B, 1, geom, on_device);
}

int smpc_set_scene_clock(smpc_handle* h, const int64_t* d_clock) {
    if (!h) return SMPC_EINVAL;
    h->scene_clock = d_clock;      // (read by the kernels when they run, never here)
    return SMPC_OK;
}

int smpc_set_instance_curves(smpc_handle* h, int B, int64_t L, const double* curves, int on_device) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    if (!curves) { h->curves.clear(); return SMPC_OK; }
    if (B <= 0 || L < 1) return fail(h, SMPC_EINVAL, "smpc_set_instance_curves: B=%d, L=%lld: need B > 0 and L >= 1", B, (long long)L);
    const size_t n = (size_t)B * 3 * (size_t)L;
    if (!on_device) {
        // (device pointers are taken as they are: reading them back would synchronise)
        for (size_t i = 0; i < n; i++)
            if (!(curves[i] - curves[i] == 0.0))
                return fail(h, SMPC_EINVAL, "curve of instance %lld (of B=%d), axis %d, column %lld (of L=%lld) is not finite",
                            (long long)(i / (3 * (size_t)L)), B, (int)(i / (size_t)L % 3), (long long)(i % (size_t)L), (long long)L);
    }
    int rc;
    if ((rc = h->curves.room(h, n)) || (rc = h->curves.upload(h, curves, n, on_device != 0))) return rc;
    h->curves.commit(B);
    h->curves_L = L;
    return SMPC_OK;
}

int smpc_set_instance_models(smpc_handle* h, int B, const smpc_joint* joints, int on_device) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    if (!joints) { h->models.clear(); return SMPC_OK; }
    if (B <= 0) return fail(h, SMPC_EINVAL, "bad batch size");
    const int nq = h->desc.nq;
    const size_t n = (size_t)B * nq;
    if (!on_device) {
        // Kinematics and limits are the descriptor's, bit for bit: a table that moves one of them asks for something the engine does
        // not do.  (Device pointers are taken as they are -- reading them back would synchronise -- and k_model_table takes those
        // fields from the descriptor.)
        const auto same = [](const double* a, const double* b, int m) { return memcmp(a, b, sizeof(double) * m) == 0; };
        const auto finite = [](const double* a, int m) {
            for (int i = 0; i < m; i++)
                if (!(a[i] - a[i] == 0.0)) return false;
            return true;
        };
        for (size_t t = 0; t < n; t++) {
            const smpc_joint &J = joints[t], &Dj = h->desc.joints[t % nq];
            const char* bad = !same(J.R0, Dj.R0, 9)             ? "R0 differs from the descriptor's"
                              : !same(J.p0, Dj.p0, 3)           ? "p0 differs from the descriptor's"
                              : !same(J.axis, Dj.axis, 3)       ? "axis differs from the descriptor's"
                              : !same(&J.q_min, &Dj.q_min, 1)   ? "q_min differs from the descriptor's"
                              : !same(&J.q_max, &Dj.q_max, 1)   ? "q_max differs from the descriptor's"
                              : !same(&J.v_max, &Dj.v_max, 1)   ? "v_max differs from the descriptor's"
                              : !same(&J.tau_max, &Dj.tau_max, 1) ? "tau_max differs from the descriptor's"
                              : !(finite(&J.mass, 1) && J.mass >= 0.0) ? "mass is negative or not finite"
                              : !finite(J.com, 3)               ? "com is not finite"
                              : !finite(J.inertia, 6)           ? "inertia is not finite"
                                                                : nullptr;
            if (bad)
                return fail(h, SMPC_EINVAL, "smpc_set_instance_models: instance %zu (of B=%d), joint %d: %s (only mass, com and inertia are "
                            "per instance)", t / nq, B, (int)(t % nq), bad);
        }
    }
    int rc;
    if ((rc = h->models.room(h, n))) return rc;
    if (on_device) {
        hipLaunchKernelGGL(k_model_table, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, h->d_desc, (long)n, nq, joints, h->models.d.p);
        HIPCHK(h, hipGetLastError());
    } else if ((rc = h->models.upload(h, joints, n, false)))
        return rc;      // (the records as they came: their other fields have just been found equal to the descriptor's)
    h->models.commit(B);
    return SMPC_OK;
}

int smpc_solve_batch(smpc_handle* h, int B, const double* x0, const double* xg, const double* ug, const double* p,
                     double* x_out, double* u_out, int32_t* status, int32_t* qp_iter, int on_device) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || !x0 || !xg || !ug || !p || !x_out || !u_out || !status) return fail(h, SMPC_EINVAL, "bad argument");
    (void)hipSetDevice(h->device);
    int rc;
    if ((rc = guard_solve_slots(h, B, "smpc_solve_batch"))) return rc;
    if ((rc = ensure_batch(h, B))) return rc;
    const size_t nX = (size_t)B * (h->N + 1) * 2 * h->desc.nq, nU = (size_t)B * h->N * h->desc.nq;
    Stage io{h, on_device != 0};
    const double *dx0, *dxg, *dug, *dp;
    double *dxo, *duo;
    int32_t *dst, *dit;
    if ((rc = io.place([&](Stage& v) {
             dx0 = v.in(x0, (size_t)B * 2 * h->desc.nq);
             dxg = v.in(xg, nX);
             dug = v.in(ug, nU);
             dp = v.in(p, (size_t)B * (h->N + 1) * SMPC_NP);
             dxo = v.out(x_out, nX);
             duo = v.out(u_out, nU);
             dst = v.out(status, (size_t)B);
             dit = v.out(qp_iter, (size_t)B);
         })))
        return rc;
    if ((rc = with_nq(h, [&](auto NQ) { return launch_solve<NQ>(h, B, dx0, dxg, dug, dp, dxo, duo, dst, dit); }))) return rc;
    return io.finish();
}

int smpc_eval_nodes(smpc_handle* h, int B, const double* xg, const double* ug, const double* p, smpc_node_eval* out,
                    int on_device) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || !xg || !ug || !p || !out) return fail(h, SMPC_EINVAL, "bad argument");
    (void)hipSetDevice(h->device);
    int rc;
    if ((rc = guard_scene_context_and_models(h, B, "smpc_eval_nodes"))) return rc;
    if ((rc = ensure_batch(h, B))) return rc;
    const int N = h->N, nx = 2 * h->desc.nq, nu = h->desc.nq;
    hipStream_t s = h->stream;
    const long nodes = (long)B * (N + 1);
    Stage io{h, on_device != 0};
    const double *dxg, *dug, *dp;
    smpc_node_eval* dout;
    if ((rc = io.place([&](Stage& v) {
             dxg = v.in(xg, (size_t)nodes * nx);
             dug = v.in(ug, (size_t)B * N * nu);
             dp = v.in(p, (size_t)nodes * SMPC_NP);
             dout = v.out(out, (size_t)nodes);
         })))
        return rc;
    // (entries no kernel writes -- the unused tails of the MAX_NQ / MAX_ROWS arrays -- read as zero)
    HIPCHK(h, hipMemsetAsync(h->d_ev.p, 0, sizeof(double) * ev_tiles((size_t)nodes) * EV_TILE * EV_D, s));
    if ((rc = with_nq(h, [&](auto NQ) { return launch_eval<NQ>(h, B, dxg, dug, dp, h->d_ev.p); }))) return rc;
    hipLaunchKernelGGL(k_ev_untile, dim3((unsigned)((nodes * EV_D + 255) / 256)), dim3(256), 0, s, nodes, h->d_ev.p,
                       reinterpret_cast<double*>(dout));
    HIPCHK(h, hipGetLastError());
    return io.finish();
}

int smpc_guess_correction(smpc_handle* h, int B, double* xg, const double* ug, int on_device) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || !xg || !ug) return fail(h, SMPC_EINVAL, "bad argument");
    (void)hipSetDevice(h->device);
    const int N = h->N, nq = h->desc.nq, nx = 2 * nq;
    Stage io{h, on_device != 0};
    double* dx;
    const double* du;
    int rc;
    if ((rc = io.place([&](Stage& v) {
             dx = v.inout(xg, (size_t)B * (N + 1) * nx);
             du = v.in(ug, (size_t)B * N * nq);
         })))
        return rc;
    hipLaunchKernelGGL(k_guess_correction, dim3((B * nq + 63) / 64), dim3(64), 0, h->stream, B, N, nq, h->desc.dt, dx, du,
                       (const uint8_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
    HIPCHK(h, hipGetLastError());
    return io.finish();
}

int smpc_provide_control(smpc_handle* h, int B, const int32_t* accept, const double* x_temp, const double* u_temp,
                         double* xg, double* ug, double* u_apply, int on_device) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || !accept || !x_temp || !u_temp || !xg || !ug || !u_apply) return fail(h, SMPC_EINVAL, "bad argument");
    (void)hipSetDevice(h->device);
    const int N = h->N, nq = h->desc.nq, nx = 2 * nq;
    const size_t nX = (size_t)B * (N + 1) * nx, nU = (size_t)B * N * nq;
    Stage io{h, on_device != 0};
    const int32_t* dacc;
    const double *dxt, *dut;
    double *dxg, *dug, *dua;
    int rc;
    if ((rc = io.place([&](Stage& v) {
             dxt = v.in(x_temp, nX);
             dut = v.in(u_temp, nU);
             dxg = v.inout(xg, nX);
             dug = v.inout(ug, nU);
             dua = v.out(u_apply, (size_t)B * nq);
             dacc = v.in(accept, (size_t)B);
         })))
        return rc;
    hipLaunchKernelGGL(k_provide_control, dim3((B * (nx + nq) + 63) / 64), dim3(64), 0, h->stream, B, N, nq, dacc, dxt, dut, dxg, dug,
                       dua, (const uint8_t*)nullptr, (const uint8_t*)nullptr, (const double*)nullptr);
    HIPCHK(h, hipGetLastError());
    return io.finish();
}

int smpc_check_trajectory(smpc_handle* h, int B, int n_nodes, const double* x, const double* x_min, const double* x_max,
                          double tol_x, const double* row_lb_chk, const double* row_ub_chk, double alpha, double tol_safe,
                          int32_t* state_ok, int32_t* nn_ok, int on_device) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || n_nodes <= 0 || !x || !x_min || !x_max || !state_ok) return fail(h, SMPC_EINVAL, "bad argument");
    if (h->desc.n_rows > 0 && (!row_lb_chk || !row_ub_chk)) return fail(h, SMPC_EINVAL, "row check bounds missing");
    if (nn_ok && h->net->nlayers == 0) return fail(h, SMPC_ESTATE, "nn_ok requested but smpc_set_mlp was not called");
    (void)hipSetDevice(h->device);
    const size_t M = (size_t)B * n_nodes;
    // (x_min / x_max / row bounds are host pointers on both paths: small, constant per caller)
    int rc;
    if ((rc = guard_scene_and_context(h, B, "smpc_check_trajectory"))) return rc;
    if ((rc = upload_check_bounds(h, x_min, x_max, row_lb_chk, row_ub_chk))) return rc;
    Stage io{h, on_device != 0};
    const double* dx;
    int32_t *dok, *dnn;
    if ((rc = io.place([&](Stage& v) {
             dx = v.in(x, M * 2 * h->desc.nq);
             dok = v.out(state_ok, (size_t)B);
             dnn = v.out(nn_ok, M);
         })))
        return rc;
    if ((rc = check_nodes_dev(h, B, n_nodes, dx, tol_x, n_nodes, alpha, tol_safe, dok, nn_ok ? dnn : nullptr))) return rc;
    return io.finish();
}

int smpc_plant_step(smpc_handle* h, int B, const double* x, const double* u, const smpc_joint* joints_noisy,
                    const double* tau_noise, double* x_next, double* u_eff, int on_device) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || !x || !u || !x_next) return fail(h, SMPC_EINVAL, "bad argument");
    (void)hipSetDevice(h->device);
    const int nq = h->desc.nq, nx = 2 * nq;
    hipStream_t s = h->stream;
    Stage io{h, on_device != 0};
    const double *dx, *du, *dn;
    const smpc_joint* dj;
    double *dxn, *due;
    int rc;
    if ((rc = io.place([&](Stage& v) {
             dx = v.in(x, (size_t)B * nx);
             du = v.in(u, (size_t)B * nq);
             dn = v.in(tau_noise, (size_t)B * nq);
             dj = v.in(joints_noisy, (size_t)B * nq);
             dxn = v.out(x_next, (size_t)B * nx);
             due = v.out(u_eff, (size_t)B * nq);
         })))
        return rc;
    if ((rc = with_nq(h, [&](auto NQ) {
             constexpr int per = 64 / (NQ + 2);      // instances per block: PER of k_plant_step (9, 8, 7)
             hipLaunchKernelGGL((k_plant_step<NQ>), dim3((B + per - 1) / per), dim3(64), 0, s, h->d_desc, B, dx, du, dj, dn, dxn, due);
             return SMPC_OK;
         })))
        return rc;
    HIPCHK(h, hipGetLastError());
    return io.finish();
}

int smpc_rollout_batch(smpc_handle* h, int B, int n_steps, const double* x0, double* x_guess, double* u_guess,
                       const double* p, const smpc_joint* joints_noisy, const double* tau_noise, double* x_traj,
                       double* u_traj, int32_t* status_traj, int32_t* iter_traj, int on_device) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || n_steps <= 0 || !x0 || !x_guess || !u_guess || !p || !x_traj || !u_traj || !status_traj)
        return fail(h, SMPC_EINVAL, "bad argument");
    if (const int rf = refuse_slots(h, "smpc_rollout_batch", "the worker handles of the rollout hold none (step the loop through smpc_policy_step / "
                                    "smpc_loop_post instead)", {&h->scene, &h->ctx, &h->models, &h->rowb}))
        return rf;
    (void)hipSetDevice(h->device);
    const int N = h->N, nq = h->desc.nq, nx = 2 * nq;
    hipStream_t s = h->stream;
    int rc;
    const size_t nX = (size_t)B * (N + 1) * nx, nU = (size_t)B * N * nq, nP = (size_t)B * (N + 1) * SMPC_NP;
    const size_t sx = (size_t)B * nx, su = (size_t)B * nq;
    Stage io{h, on_device != 0};
    const double *dx0, *dp, *dnoise;
    const smpc_joint* dj;
    double *dxg, *dug, *dxt, *dut;
    int32_t *dst, *dit;
    if ((rc = io.place([&](Stage& v) {
             dx0 = v.in(x0, sx);
             dxg = v.inout(x_guess, nX);
             dug = v.inout(u_guess, nU);
             dp = v.in(p, nP);
             dxt = v.out(x_traj, sx * (n_steps + 1));
             dut = v.out(u_traj, su * n_steps);
             dj = v.in(joints_noisy, (size_t)B * nq);
             dnoise = v.in(tau_noise, su * n_steps);
             dst = v.out(status_traj, (size_t)B * n_steps);
             dit = v.out(iter_traj, (size_t)B * n_steps);
         })))
        return rc;
    // ---- the steps.  Instances are independent, so a large batch is split into sub-batches that advance on their own
    // streams (worker handles): while one sub-batch's QP launch waits for its slowest instances the others' kernels fill the
    // chip (scripts/rollout_bench.py, B = 4096, round 4: 3.53 / 3.06 / 3.04 / 3.07 ms per step with 1 / 2 / 3 / 4 sub-batches,
    // twice on one box; the Python-driven three-stream loop of bench.py: 2.9 over the same 40 steps).  Results are the same bits
    // whatever the split.
    int n_sub = B >= 3072 ? 3 : (B >= 1024 ? 2 : 1);
    if (const char* ev = getenv("SMPC_ROLLOUT_STREAMS")) n_sub = atoi(ev);
    if (n_sub < 1) n_sub = 1;
    if (n_sub > B) n_sub = B;
    if (h->bounds.for_batch(B)) n_sub = 1;                      // per-instance stage bounds are held by this handle only
    // (workspaces are allocated by whoever solves: the workers below when the batch is split -- the parent then holds none of
    //  the QP workspace / linearisation records of the full batch -- otherwise this handle)
    rc = SMPC_OK;
    hipError_t e = hipMemcpyAsync(dxt, dx0, sizeof(double) * sx, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return fail(h, SMPC_EHIP, "rollout init failed: %s", hipGetErrorString(e));
    if (n_sub > 1) {
        h->timed = 0;      // (the solves run on the workers: smpc_get_timing on this handle reports "nothing timed", not stale numbers)
        if ((rc = rollout_workers(h, n_sub))) return rc;
        if (!h->ev_fork) HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
        HIPCHK(h, hipEventRecord(h->ev_fork, s));        // inputs (staging copies, x_traj[0]) are ordered before the workers
    }
    struct Slice { smpc_handle* w; int lo, n; RollScratch r; };
    std::vector<Slice> slices;
    for (int k = 0; k < n_sub; k++) {
        const int base = B / n_sub, rem = B % n_sub;
        const int lo = k * base + (k < rem ? k : rem), n = base + (k < rem ? 1 : 0);
        smpc_handle* w = n_sub > 1 ? h->kids[k] : h;
        if (n_sub > 1) HIPCHK(h, hipStreamWaitEvent(w->stream, h->ev_fork, 0));
        const int nn_mode = h->desc.nn_mode;
        w->mlp_rows_whole = n_sub > 1 ? (nn_mode == SMPC_NN_TERMINAL ? (long)B : (long)B * N) : 0;
        int rw;
        if ((rw = ensure_batch(w, n)) || (rw = w->d_roll.reserve(w, "rollout scratch", roll_layout(nullptr, n, N, nq).bytes)))
            return fail(h, rw, "worker %d: %s", k, w->err);
        const RollScratch r = roll_layout(w->d_roll.p, n, N, nq);
        if (hipMemsetAsync(r.fails, 0, sizeof(int32_t) * n, w->stream) != hipSuccess) return fail(h, SMPC_EHIP, "rollout init failed");
        slices.push_back({w, lo, n, r});
    }
    for (int t = 0; t < n_steps && rc == SMPC_OK; t++) {
        for (const Slice& sl : slices) {
            smpc_handle* w = sl.w;
            const int lo = sl.lo, n = sl.n;
            double* xt = dxt + (size_t)t * sx + (size_t)lo * nx;
            double* ut = dut + (size_t)t * su + (size_t)lo * nq;
            double* xg_w = dxg + (size_t)lo * (N + 1) * nx;
            double* ug_w = dug + (size_t)lo * N * nq;
            const double* p_w = dp + (size_t)lo * (N + 1) * SMPC_NP;
            int32_t* st_w = dst + (size_t)t * B + lo;
            int32_t* it_w = dit ? dit + (size_t)t * B + lo : sl.r.it;
            if ((rc = smpc_guess_correction(w, n, xg_w, ug_w, 1))) break;
            if ((rc = smpc_solve_batch(w, n, xt, xg_w, ug_w, p_w, sl.r.xo, sl.r.uo, st_w, it_w, 1))) break;
            hipLaunchKernelGGL(k_accept, dim3((n + 63) / 64), dim3(64), 0, w->stream, n, st_w, sl.r.fails, sl.r.accept);
            if ((rc = smpc_provide_control(w, n, sl.r.accept, sl.r.xo, sl.r.uo, xg_w, ug_w, ut, 1))) break;
            rc = smpc_plant_step(w, n, xt, ut, dj ? dj + (size_t)lo * nq : nullptr,
                                 dnoise ? dnoise + (size_t)t * su + (size_t)lo * nq : nullptr, xt + sx, nullptr, 1);
            if (rc) break;
        }
        if (rc && n_sub > 1) for (const Slice& sl : slices) if (sl.w->err[0]) snprintf(h->err, sizeof(h->err), "%s", sl.w->err);
    }
    if (n_sub > 1) {      // join: this handle's stream (copy-back, the caller's smpc_sync) comes after every worker
        if (!h->ev_join) HIPCHK(h, hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
        for (const Slice& sl : slices) {
            HIPCHK(h, hipEventRecord(h->ev_join, sl.w->stream));
            HIPCHK(h, hipStreamWaitEvent(s, h->ev_join, 0));
        }
    }
    if (rc) {
        if (!on_device) (void)hipStreamSynchronize(s);      // (host path: nothing of the call is in flight on return)
        return rc;
    }
    return io.finish();
}

// ---- the policy layer on the device ------------------------------------------------------------------------------------------
int smpc_policy_step(smpc_handle* h, int B, const smpc_policy_params* par, const smpc_policy_state* st, const double* x,
                     const uint8_t* stepping, const double* u_other, double* u_out, uint8_t* abort_out, int32_t* any_abort) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || !par || !st || !x || !u_out || !abort_out || !any_abort) return fail(h, SMPC_EINVAL, "bad argument");
    if (!st->x_guess || !st->u_guess || !st->x_temp || !st->u_temp || !st->p || !st->x_viable || !st->fails ||
        !st->current_step || !st->status || !st->qp_iter)
        return fail(h, SMPC_EINVAL, "policy state incomplete");
    const int kind = par->kind;
    if (kind < SMPC_POLICY_NAIVE || kind > SMPC_POLICY_PARALLEL) return fail(h, SMPC_EINVAL, "unknown policy kind %d", kind);
    const bool receding = kind == SMPC_POLICY_RECEDING || kind == SMPC_POLICY_REAL_RECEDING;
    const bool parallel = kind == SMPC_POLICY_PARALLEL;
    if ((receding || parallel) && !st->r) return fail(h, SMPC_EINVAL, "receding policy without r");
    if (parallel && h->desc.nn_mode != SMPC_NN_ALL) return fail(h, SMPC_EINVAL, "parallel policy needs the safe-set row on every node (SMPC_NN_ALL)");
    if (kind == SMPC_POLICY_REAL_RECEDING && (!par->stage_lo || !par->stage_hi)) return fail(h, SMPC_EINVAL, "stage_lo / stage_hi missing");
    if (stepping && !u_other) return fail(h, SMPC_EINVAL, "u_other missing");
    if (kind != SMPC_POLICY_NAIVE && (!par->x_min || !par->x_max || (h->desc.n_rows > 0 && (!par->row_lb_chk || !par->row_ub_chk))))
        return fail(h, SMPC_EINVAL, "check bounds missing");
    if ((receding || parallel) && h->net->nlayers == 0) return fail(h, SMPC_ESTATE, "receding policy but smpc_set_mlp was not called");
    if (parallel)
        if (const int rf = refuse_slots(h, "smpc_policy_step", "the parallel policy's candidate slots are not instances",
                                            {&h->scene, &h->ctx, &h->models, &h->rowb}))
            return rf;
    (void)hipSetDevice(h->device);
    const int N = h->N, nq = h->desc.nq, nx = 2 * nq;
    hipStream_t s = h->stream;
    int rc;
    if ((rc = guard_solve_slots(h, B, "smpc_policy_step"))) return rc;
    TrajSrc tr;
    if (!parallel && (rc = policy_traj_src(h, B, st, &tr))) return rc;     // (before anything is enqueued; the parallel step asks itself)
    if ((rc = ensure_batch(h, B))) return rc;
    PolScratch w;
    if ((rc = policy_scratch(h, B, &w))) return rc;
    int32_t *d_ok = w.ok, *d_safe = w.safe, *d_acc = w.acc;
    uint8_t* d_act = w.act;
    if (kind != SMPC_POLICY_NAIVE && (rc = upload_check_bounds(h, par->x_min, par->x_max, par->row_lb_chk, par->row_ub_chk))) return rc;
    if (parallel) return policy_step_parallel(h, B, par, st, x, stepping, u_other, u_out, abort_out, any_abort, d_ok, d_safe, d_acc, d_act);
    // guessCorrection (not RealReceding, controller.py:524-565); the launch also resets *any_abort.  Every kind launches exactly
    // one of the two kernels that do so -- k_guess_correction here, k_policy_pre (RealReceding) below -- and both grids are
    // non-empty (B > 0, nq > 0), so thread 0 of block 0 always exists.
    if (kind != SMPC_POLICY_REAL_RECEDING)
        hipLaunchKernelGGL(k_guess_correction, dim3((B * nq + 63) / 64), dim3(64), 0, s, B, N, nq, h->desc.dt, st->x_guess,
                           st->u_guess, stepping, any_abort, d_ok);
    if (receding) {
        if (kind == SMPC_POLICY_REAL_RECEDING) {
            // (zeroed when grown: instances that never step keep valid bounds)
            if ((rc = ensure_instance_bounds(h, B, true))) return rc;
            h->bounds.commit(B);
        }
        hipLaunchKernelGGL(k_policy_pre, dim3((unsigned)(((size_t)B * (N + 1) + 63) / 64)), dim3(64), 0, s, B, N, nx, kind,
                           stepping, st->r, st->p, st->x_guess, par->stage_lo, par->stage_hi, par->tube, h->bounds.d.p, instance_hi(h),
                           kind == SMPC_POLICY_REAL_RECEDING ? any_abort : (int32_t*)nullptr,
                           kind == SMPC_POLICY_REAL_RECEDING ? d_ok : (int32_t*)nullptr);
    }
    if (tr.p)            // controller.py:153-156: the nodes' reference points follow the step counter
        hipLaunchKernelGGL(k_policy_traj, dim3((unsigned)(((size_t)B * (N + 1) + 63) / 64)), dim3(64), 0, s, B, N, stepping,
                           st->current_step, tr.p, tr.len, tr.stride, st->p);
    HIPCHK(h, hipGetLastError());
    h->d_active = stepping;
    // (the receding policies carry the row at node r and at the end node, and test nodes r + 2 .. N afterwards -- in steady state one or
    //  two per instance: their compacted lists are short, whatever their capacity)
    h->mlp_rows_hint = receding ? 2L * B : 0L;
    rc = with_nq(h, [&](auto NQ) { return launch_solve<NQ>(h, B, x, st->x_guess, st->u_guess, st->p, st->x_temp, st->u_temp, st->status, st->qp_iter); });
    h->d_active = nullptr;
    if (rc) { h->mlp_rows_hint = 0; return rc; }
    if (kind != SMPC_POLICY_NAIVE) {
        // checkStateConstraints(x_temp) (+ checkSafeConstraints(x_temp) on every node for the receding policies)
        const int coll = par->collision_first_node ? 1 : N + 1;
        if (receding) {
            // the safe-set test is only ever read at nodes r + 2 .. N of the stepping instances (k_policy_post): list them
            const size_t M = (size_t)B * (N + 1);
            if ((rc = ensure_nn_idx(h, M))) return rc;
            hipLaunchKernelGGL(k_policy_safe_list, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, s, B, N, par->abort_flag, stepping, st->r,
                               h->d_nn_idx.p, h->d_nn_cnt);
        }
        if ((rc = check_nodes_dev(h, B, N + 1, st->x_temp, par->tol_x, coll, par->alpha, par->tol_safe, d_ok, receding ? d_safe : nullptr,
                                  receding, true))) {
            h->mlp_rows_hint = 0;
            return rc;
        }
    }
    h->mlp_rows_hint = 0;
    hipLaunchKernelGGL(k_policy_post, dim3((B + 63) / 64), dim3(64), 0, s, B, N, nx, kind, par->abort_flag, stepping, st->status,
                       d_ok, d_safe, st->x_guess, st->fails, st->current_step, st->r, st->x_viable, d_acc, d_act, abort_out, any_abort,
                       (receding && kind != SMPC_POLICY_NAIVE) ? h->d_nn_cnt : (int32_t*)nullptr);

    hipLaunchKernelGGL(k_provide_control, dim3((B * (nx + nq) + 63) / 64), dim3(64), 0, s, B, N, nq, d_acc, st->x_temp, st->u_temp,
                       st->x_guess, st->u_guess, u_out, stepping, d_act, u_other);
    HIPCHK(h, hipGetLastError());
    return SMPC_OK;
}

int smpc_loop_pre(smpc_handle* h, int B, int Nb, const smpc_loop_state* ls, const int64_t* r, const uint8_t* pending, double* u_other,
                  uint8_t* stepping) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || Nb <= 0 || !ls || !u_other || !stepping) return fail(h, SMPC_EINVAL, "bad argument");
    if (!ls->x_cur || !ls->alive || !ls->sa || !ls->ja || !ls->x_abort || !ls->u_abort || !ls->step)
        return fail(h, SMPC_EINVAL, "loop state incomplete");
    (void)hipSetDevice(h->device);
    hipLaunchKernelGGL(k_loop_pre, dim3((B + 63) / 64), dim3(64), 0, h->stream, B, h->desc.nq, Nb, ls->x_cur, ls->alive, ls->sa,
                       ls->ja, ls->x_abort, ls->u_abort, r, ls->step, ls->r_log, u_other, stepping, pending, ls->resumed);
    HIPCHK(h, hipGetLastError());
    return SMPC_OK;
}

int smpc_loop_classify_aborts(smpc_handle* h, int B, const smpc_loop_state* ls, int reference_quirks, uint8_t* abort,
                              int32_t* any_event) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || !ls || !abort || !any_event) return fail(h, SMPC_EINVAL, "bad argument");
    if (!ls->sa) return fail(h, SMPC_EINVAL, "loop state incomplete");
    (void)hipSetDevice(h->device);
    HIPCHK(h, hipMemsetAsync(any_event, 0, sizeof(int32_t), h->stream));
    hipLaunchKernelGGL(k_loop_classify_aborts, dim3((B + 63) / 64), dim3(64), 0, h->stream, B, reference_quirks, ls->resumed,
                       ls->sa, abort, any_event);
    HIPCHK(h, hipGetLastError());
    return SMPC_OK;
}

int smpc_loop_apply_backup(smpc_handle* h, int B, int Nb, const smpc_loop_state* ls, int n_c, const int64_t* rows,
                           const int32_t* status_c, const double* x_c, const double* u_c, uint8_t* viable, double* u,
                           uint8_t* pending) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || Nb <= 0 || n_c < 0 || n_c > B || !ls || !viable || !u || !pending) return fail(h, SMPC_EINVAL, "bad argument");
    if (n_c == 0) return SMPC_OK;
    if (!rows || !status_c || !x_c || !u_c) return fail(h, SMPC_EINVAL, "bad argument");
    if (!ls->x_cur || !ls->alive || !ls->sa || !ls->collided || !ls->ja || !ls->last_x || !ls->last_u || !ls->x_abort ||
        !ls->u_abort || !ls->step)
        return fail(h, SMPC_EINVAL, "loop state incomplete");
    (void)hipSetDevice(h->device);
    hipLaunchKernelGGL(k_loop_apply_backup, dim3((n_c + 63) / 64), dim3(64), 0, h->stream, n_c, h->desc.nq, Nb, rows, status_c, x_c, u_c,
                       ls->x_cur, ls->step, ls->alive, ls->sa, ls->collided, viable, ls->ja, ls->last_x, ls->last_u, ls->x_abort,
                       ls->u_abort, u, pending);
    HIPCHK(h, hipGetLastError());
    return SMPC_OK;
}

int smpc_loop_post(smpc_handle* h, int B, const smpc_policy_params* par, const smpc_loop_state* ls, const double* u,
                   const smpc_joint* joints_noisy, const double* tau_noise) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || !par || !ls || !u) return fail(h, SMPC_EINVAL, "bad argument");
    if (!ls->x_cur || !ls->alive || !ls->collided || !ls->last_x || !ls->last_u || !ls->step || !ls->x_log || !ls->u_log)
        return fail(h, SMPC_EINVAL, "loop state incomplete");
    if (!par->x_min || !par->x_max || (h->desc.n_rows > 0 && (!par->row_lb_chk || !par->row_ub_chk)))
        return fail(h, SMPC_EINVAL, "check bounds missing");
    (void)hipSetDevice(h->device);
    const int nq = h->desc.nq;
    hipStream_t s = h->stream;
    int rc;
    if ((rc = h->scene.guard(h, B, "smpc_loop_post")) || (rc = h->world.guard(h, B, "smpc_loop_post"))) return rc;
    PolScratch w;       // (its x_next [B][nx] and ok [B] lie behind smpc_policy_step's part)
    if ((rc = policy_scratch(h, B, &w))) return rc;
    if ((rc = upload_check_bounds(h, par->x_min, par->x_max, par->row_lb_chk, par->row_ub_chk))) return rc;
    if ((rc = smpc_plant_step(h, B, ls->x_cur, u, joints_noisy, tau_noise, w.xn, nullptr, 1))) return rc;
    // one node per instance: the model bounds widened by tol_x and the rows against their check bounds = checkStateConstraints
    if ((rc = check_nodes_dev(h, B, 1, w.xn, par->tol_x, 1, 0.0, 0.0, w.okn, nullptr, false, false, 1))) return rc;
    hipLaunchKernelGGL(k_loop_post, dim3((B + 63) / 64), dim3(64), 0, s, B, nq, u, w.xn, w.okn, ls->step, ls->x_log, ls->u_log,
                       ls->alive, ls->collided, ls->last_x, ls->last_u, ls->x_cur);
    hipLaunchKernelGGL(k_step_advance, dim3(1), dim3(1), 0, s, ls->step);
    HIPCHK(h, hipGetLastError());
    return SMPC_OK;
}

// ---- SQP with merit backtracking ---------------------------------------------------------------------------------------------------
int smpc_merit_terms(smpc_handle* h, int B, const double* x0, const double* x, const double* u, const double* p, const double* dx,
                     const double* du, const double* alpha, const uint8_t* mask, double* out, int on_device) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || !x0 || !x || !u || !p || !out) return fail(h, SMPC_EINVAL, "bad argument");
    if ((dx == nullptr) != (du == nullptr)) return fail(h, SMPC_EINVAL, "dx and du must both be given or both be NULL");
    if (alpha && !dx) return fail(h, SMPC_EINVAL, "alpha without a step");
    (void)hipSetDevice(h->device);
    const int N = h->N, nq = h->desc.nq;
    const size_t nX = (size_t)B * (N + 1) * 2 * nq, nU = (size_t)B * N * nq;
    int rc;
    if ((rc = guard_solve_slots(h, B, "smpc_merit_terms"))) return rc;
    SqpScratch w;
    if ((rc = sqp_scratch(h, B, false, &w))) return rc;
    Stage io{h, on_device != 0};
    const double *dx0, *dxg, *dug, *dp, *ddx, *ddu, *dal;
    const uint8_t* dmask;
    double* dout;
    if ((rc = io.place([&](Stage& v) {
             dx0 = v.in(x0, (size_t)B * 2 * nq);
             dxg = v.in(x, nX);
             dug = v.in(u, nU);
             dp = v.in(p, (size_t)B * (N + 1) * SMPC_NP);
             ddx = v.in(dx, nX);
             ddu = v.in(du, nU);
             dal = v.in(alpha, (size_t)B);
             dmask = v.in(mask, (size_t)B);
             dout = v.inout(out, (size_t)3 * B);
         })))
        return rc;
    if ((rc = with_nq(h, [&](auto NQ) { return launch_merit<NQ>(h, B, w, dx0, dxg, dug, dp, ddx, ddu, dal, dmask, dout); }))) return rc;
    return io.finish();
}

int smpc_sqp_batch(smpc_handle* h, int B, const smpc_sqp_opts* opts, const double* x0, double* x_guess, double* u_guess,
                   const double* p, const smpc_sqp_state* state, int on_device) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || !opts || !x0 || !x_guess || !u_guess || !p || !state) return fail(h, SMPC_EINVAL, "bad argument");
    if (!state->mu || !state->done || !state->status || !state->alpha || !state->merit_before || !state->merit || !state->violation ||
        !state->updated || !state->iters || !state->qp_iter_total)
        return fail(h, SMPC_EINVAL, "SQP state incomplete");
    if (opts->max_iter < 0 || !(opts->alpha_reduction > 0.0 && opts->alpha_reduction < 1.0) || !(opts->alpha_min > 0.0 && opts->alpha_min <= 1.0))
        return fail(h, SMPC_EINVAL, "SQP options: max_iter >= 0, 0 < alpha_reduction < 1, 0 < alpha_min <= 1");
    (void)hipSetDevice(h->device);
    const int N = h->N, nq = h->desc.nq;
    const int nX1 = (N + 1) * 2 * nq, nU1 = N * nq;
    const size_t nX = (size_t)B * nX1, nU = (size_t)B * nU1;
    hipStream_t s = h->stream;
    int rc;
    if ((rc = guard_solve_slots(h, B, "smpc_sqp_batch"))) return rc;
    if ((rc = ensure_batch(h, B, false))) return rc;
    SqpScratch w;
    if ((rc = sqp_scratch(h, B, true, &w))) return rc;
    Stage io{h, on_device != 0};
    const double *dx0, *dp;
    double *dxg, *dug, *d_mu, *d_alpha, *d_before, *d_merit, *d_viol;
    uint8_t *d_done, *d_upd;
    int32_t *d_status, *d_iters, *d_qpit;
    if ((rc = io.place([&](Stage& v) {
             dx0 = v.in(x0, (size_t)B * 2 * nq);
             dp = v.in(p, (size_t)B * (N + 1) * SMPC_NP);
             dxg = v.inout(x_guess, nX);
             dug = v.inout(u_guess, nU);
             d_mu = v.inout(state->mu, (size_t)B);
             d_alpha = v.inout(state->alpha, (size_t)B);
             d_before = v.inout(state->merit_before, (size_t)B);
             d_merit = v.inout(state->merit, (size_t)B);
             d_viol = v.inout(state->violation, (size_t)B);
             d_done = v.inout(state->done, (size_t)B);
             d_upd = v.inout(state->updated, (size_t)B);
             d_status = v.inout(state->status, (size_t)B);
             d_iters = v.inout(state->iters, (size_t)B);
             d_qpit = v.inout(state->qp_iter_total, (size_t)B);
         })))
        return rc;
    const bool captured = capturing(h);
    const dim3 blk(64), per_inst((B + 63) / 64);
    // step lengths an instance can try: 1, r, r^2, .. while above alpha_min, then alpha_min itself
    int n_trials = 1;
    for (double a = 1.0; a > opts->alpha_min && n_trials < 64; n_trials++) a = a * opts->alpha_reduction > opts->alpha_min ? a * opts->alpha_reduction : opts->alpha_min;
    for (int iter = 0; iter < opts->max_iter; iter++) {
        hipLaunchKernelGGL(k_sqp_begin, per_inst, blk, 0, s, B, d_done, w.act, w.n_open);
        HIPCHK(h, hipGetLastError());
        h->d_active = w.act;
        rc = with_nq(h, [&](auto NQ) { return launch_solve<NQ>(h, B, dx0, dxg, dug, dp, w.xs, w.us, w.st, w.it); });
        h->d_active = nullptr;
        if (rc) return rc;
        hipLaunchKernelGGL(k_sqp_direction, dim3(B), blk, 0, s, B, nX1, nU1, w.act, dxg, dug, w.xs, w.us, w.dx, w.du, w.step);
        HIPCHK(h, hipGetLastError());
        // merit terms and grad f . d at the iterate
        if ((rc = with_nq(h, [&](auto NQ) { return launch_merit<NQ>(h, B, w, dx0, dxg, dug, dp, w.dx, w.du, nullptr, w.act, w.m0t); }))) return rc;
        hipLaunchKernelGGL(k_sqp_penalty, per_inst, blk, 0, s, B, opts->mu_max, w.act, w.st, w.it, w.m0t, d_mu, w.m0, w.Dd, w.alpha, w.settled,
                           w.trial, d_status, d_iters, d_qpit);
        HIPCHK(h, hipGetLastError());
        // the line search: every pass evaluates the instances not yet settled at their own step length (a pass over none costs its
        // launches only; how many instances are still searching is not read back)
        for (int t = 0; t < n_trials; t++) {
            if ((rc = with_nq(h, [&](auto NQ) { return launch_merit<NQ>(h, B, w, dx0, dxg, dug, dp, w.dx, w.du, w.alpha, w.trial, w.mt); }))) return rc;
            hipLaunchKernelGGL(k_sqp_armijo, per_inst, blk, 0, s, B, opts->armijo, opts->alpha_reduction, opts->alpha_min, w.mt, d_mu, w.m0,
                               w.Dd, w.alpha, w.settled, w.trial);
            HIPCHK(h, hipGetLastError());
        }
        hipLaunchKernelGGL(k_sqp_finish, per_inst, blk, 0, s, B, opts->tol, w.act, w.st, w.step, w.alpha, d_mu, w.m0, w.m0t, w.mt, d_done, d_upd,
                           d_alpha, d_before, d_merit, d_viol, w.n_open);
        hipLaunchKernelGGL(k_sqp_commit, dim3((unsigned)(((size_t)B * (nX1 + nU1) + 63) / 64)), blk, 0, s, B, nX1, nU1, w.act, d_upd, d_alpha,
                           w.dx, w.du, dxg, dug);
        HIPCHK(h, hipGetLastError());
        if (!captured && iter + 1 < opts->max_iter) {
            int32_t open = 0;
            HIPCHK(h, hipMemcpyAsync(&open, w.n_open, sizeof(open), hipMemcpyDeviceToHost, s));
            HIPCHK(h, hipStreamSynchronize(s));
            if (open == 0) break;
        }
    }
    return io.finish();
}

int smpc_check_guess(smpc_handle* h, int B, const double* x, const double* u, const smpc_guess_check* par, const uint8_t* mask,
                     int32_t* flags, double* worst, int on_device) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || !x || !u || !par || !flags || !worst) return fail(h, SMPC_EINVAL, "bad argument");
    if (!par->x_min || !par->x_max || !par->tau_min || !par->tau_max) return fail(h, SMPC_EINVAL, "state or torque bounds missing");
    if (h->desc.n_rows > 0 && (!par->row_lb_chk || !par->row_ub_chk)) return fail(h, SMPC_EINVAL, "row check bounds missing");
    if (par->safe_node > h->N) return fail(h, SMPC_EINVAL, "safe_node=%d beyond the horizon N=%d", (int)par->safe_node, h->N);
    if (par->safe_node >= 0 && h->net->nlayers == 0) return fail(h, SMPC_ESTATE, "safe_node given but smpc_set_mlp was not called");
    (void)hipSetDevice(h->device);
    const int N = h->N, nq = h->desc.nq;
    int rc;
    if ((rc = guard_scene_context_and_models(h, B, "smpc_check_guess"))) return rc;
    if ((rc = upload_guess_bounds(h, par))) return rc;
    Stage io{h, on_device != 0};
    const double *dx, *du;
    const uint8_t* dmask;
    int32_t* dflags;
    double* dworst;
    if ((rc = io.place([&](Stage& v) {
             dx = v.in(x, (size_t)B * (N + 1) * 2 * nq);
             du = v.in(u, (size_t)B * N * nq);
             dmask = v.in(mask, (size_t)B);
             dflags = v.inout(flags, (size_t)B);
             dworst = v.inout(worst, (size_t)B * GUESS_N_WORST);
         })))
        return rc;
    if ((rc = with_nq(h, [&](auto NQ) { return launch_check_guess<NQ>(h, B, dx, du, par, dmask, dflags, dworst); }))) return rc;
    return io.finish();
}

int smpc_ray_update(smpc_handle* h, int B, const smpc_ray_opts* opts, const smpc_ray_state* rays, const smpc_sqp_state* sqp,
                    const int32_t* flags, double* x0, double* x_guess, double* u_guess, int32_t* n_open, int on_device) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || !opts || !rays || !sqp || !flags || !x0 || !x_guess || !u_guess || !n_open) return fail(h, SMPC_EINVAL, "bad argument");
    if (opts->bisect < 0 || opts->budget < 1)
        return fail(h, SMPC_EINVAL, "ray options: bisect=%d >= 0, budget=%d >= 1", (int)opts->bisect, (int)opts->budget);
    if (!rays->q || !rays->d || !rays->lo || !rays->hi || !rays->s || !rays->trial || !rays->kind || !rays->open || !rays->x_cert ||
        !rays->u_cert || !rays->iters_total)
        return fail(h, SMPC_EINVAL, "ray state incomplete");
    if (!sqp->mu || !sqp->done || !sqp->status || !sqp->alpha || !sqp->merit_before || !sqp->merit || !sqp->violation || !sqp->updated ||
        !sqp->iters || !sqp->qp_iter_total)
        return fail(h, SMPC_EINVAL, "SQP state incomplete");
    (void)hipSetDevice(h->device);
    const int N = h->N, nq = h->desc.nq;
    const size_t nX = (size_t)B * (N + 1) * 2 * nq, nU = (size_t)B * N * nq, nB = (size_t)B;
    Stage io{h, on_device != 0};
    smpc_ray_state R;
    smpc_sqp_state S;
    const int32_t* dflags;
    double *dx0, *dxg, *dug;
    int32_t* dopen;
    int rc;
    if ((rc = io.place([&](Stage& v) {
             R.q = v.in(rays->q, nB * nq);
             R.d = v.in(rays->d, nB * nq);
             R.lo = v.inout(rays->lo, nB);
             R.hi = v.inout(rays->hi, nB);
             R.s = v.inout(rays->s, nB);
             R.trial = v.inout(rays->trial, nB);
             R.kind = v.inout(rays->kind, nB);
             R.open = v.inout(rays->open, nB);
             R.x_cert = v.inout(rays->x_cert, nX);
             R.u_cert = v.inout(rays->u_cert, nU);
             R.iters_total = v.inout(rays->iters_total, nB);
             S.mu = v.inout(sqp->mu, nB);
             S.done = v.inout(sqp->done, nB);
             S.status = v.inout(sqp->status, nB);
             S.alpha = v.inout(sqp->alpha, nB);
             S.merit_before = v.inout(sqp->merit_before, nB);
             S.merit = v.inout(sqp->merit, nB);
             S.violation = v.inout(sqp->violation, nB);
             S.updated = v.inout(sqp->updated, nB);
             S.iters = v.inout(sqp->iters, nB);
             S.qp_iter_total = v.inout(sqp->qp_iter_total, nB);
             dflags = v.in(flags, nB);
             dx0 = v.inout(x0, nB * 2 * nq);
             dxg = v.inout(x_guess, nX);
             dug = v.inout(u_guess, nU);
             dopen = v.out(n_open, 1);
         })))
        return rc;
    HIPCHK(h, hipMemsetAsync(dopen, 0, sizeof(int32_t), h->stream));
    hipLaunchKernelGGL(k_ray_update, dim3(B), dim3(64), 0, h->stream, B, nq, N, *opts, R, S, dflags, dx0, dxg, dug, dopen);
    HIPCHK(h, hipGetLastError());
    return io.finish();
}

int smpc_ik_batch(smpc_handle* h, int B, int S, const double* target, const double* q_start, const smpc_ik_params* par,
                  const uint8_t* mask, double* q_out, int32_t* info, double* resid, int on_device) {
    if (!h) return SMPC_EINVAL;
    if (B <= 0 || !target || !q_start || !par || !q_out || !info || !resid) return fail(h, SMPC_EINVAL, "bad argument");
    if (S < 1 || S > IK_MAX_STARTS) return fail(h, SMPC_EINVAL, "S=%d starts per instance outside 1..%d", S, IK_MAX_STARTS);
    if (par->max_iter < 1) return fail(h, SMPC_EINVAL, "max_iter=%d: at least one iteration", (int)par->max_iter);
    if (!par->q_lo || !par->q_hi) return fail(h, SMPC_EINVAL, "joint bounds missing");
    if (h->desc.n_rows > 0 && (!par->row_lb || !par->row_ub)) return fail(h, SMPC_EINVAL, "row bounds missing");
    (void)hipSetDevice(h->device);
    const int nq = h->desc.nq;
    int rc;
    if ((rc = h->scene.guard(h, B, "smpc_ik_batch"))) return rc;
    if ((rc = upload_ik_bounds(h, par))) return rc;
    Stage io{h, on_device != 0};
    const double *dt, *dq;
    const uint8_t* dmask;
    double *dqo, *dres;
    int32_t* dinfo;
    if ((rc = io.place([&](Stage& v) {
             dt = v.in(target, (size_t)B * 3);
             dq = v.in(q_start, (size_t)B * S * nq);
             dmask = v.in(mask, (size_t)B);
             dqo = v.inout(q_out, (size_t)B * nq);
             dinfo = v.inout(info, (size_t)B * 2);
             dres = v.inout(resid, (size_t)B * 2);
         })))
        return rc;
    if ((rc = with_nq(h, [&](auto NQ) { return launch_ik<NQ>(h, B, S, dt, dq, par, dmask, dqo, dinfo, dres); }))) return rc;
    return io.finish();
}

int smpc_score_rollout(smpc_handle* h, int B, int n_steps, const double* x_log, const double* u_log, const int64_t* last_x,
                       const int64_t* last_u, const smpc_score_params* par, const uint8_t* mask, double* out, int32_t* outi,
                       int on_device) {
    if (!h) return SMPC_EINVAL;
    if (n_steps < 1) return fail(h, SMPC_EINVAL, "n_steps=%d: a log has at least one step", n_steps);
    if (B <= 0 || !x_log || !u_log || !par || !out || !outi) return fail(h, SMPC_EINVAL, "bad argument");
    if (!par->x_min || !par->x_max) return fail(h, SMPC_EINVAL, "state bounds missing");
    if (h->desc.n_rows > 0 && (!par->row_lb_chk || !par->row_ub_chk)) return fail(h, SMPC_EINVAL, "row check bounds missing");
    if (par->traj && par->traj_len < 1) return fail(h, SMPC_EINVAL, "traj given with traj_len=%lld", (long long)par->traj_len);
    // neither pointer: the reference of instance b is its own curve (smpc_set_instance_curves), if the handle holds curves
    const bool own = !par->traj && !par->ee_ref && h->curves.B;
    if (!par->traj && !par->ee_ref && !own) return fail(h, SMPC_EINVAL, "neither ee_ref nor traj given");
    if (par->want_safe && h->net->nlayers == 0) return fail(h, SMPC_ESTATE, "want_safe given but smpc_set_mlp was not called");
    (void)hipSetDevice(h->device);
    const int nq = h->desc.nq;
    int rc;
    if ((rc = guard_scene_and_context(h, B, "smpc_score_rollout"))) return rc;
    if (own && (rc = h->curves.guard(h, B, "smpc_score_rollout"))) return rc;
    if ((rc = upload_score_bounds(h, par))) return rc;
    Stage io{h, on_device != 0};
    const double *dx, *du, *dtraj;
    const int64_t *dlx, *dlu;
    const uint8_t* dmask;
    double* dout;
    int32_t* douti;
    if ((rc = io.place([&](Stage& v) {
             dx = v.in(x_log, (size_t)(n_steps + 1) * B * 2 * nq);
             du = v.in(u_log, (size_t)n_steps * B * nq);
             dlx = v.in(last_x, (size_t)B);
             dlu = v.in(last_u, (size_t)B);
             dtraj = v.in(par->traj, (size_t)3 * (par->traj ? par->traj_len : 0));
             dmask = v.in(mask, (size_t)B);
             dout = v.inout(out, (size_t)B * SCORE_ND);
             douti = v.inout(outi, (size_t)B * SCORE_NI);
         })))
        return rc;
    const double* ref = own ? h->curves.held() : dtraj;
    const long ref_len = own ? (long)h->curves_L : (long)par->traj_len, ref_stride = own ? 3 * (long)h->curves_L : 0L;
    if ((rc = with_nq(h, [&](auto NQ) { return launch_score<NQ>(h, B, n_steps, dx, du, dlx, dlu, par, ref, ref_len, ref_stride, dmask, dout, douti); })))
        return rc;
    return io.finish();
}

int smpc_sync(smpc_handle* h) {
    if (!h) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SMPC_OK;
}

void* smpc_stream(smpc_handle* h) { return h ? (void*)h->stream : nullptr; }

int smpc_enable_timing(smpc_handle* h, int on) {
    if (!h) return SMPC_EINVAL;
    h->timing = on == 2 ? 2 : (on ? 1 : 0);
    h->timed = 0;
    h->timed_count = 0;
    for (bool& c : h->ev_complete) c = false;
    if (h->timing != 1) return SMPC_OK;
    (void)hipSetDevice(h->device);
    return h->d_wstat.reserve(h, "load-balance probe", 4 * sizeof(unsigned long long));
}

int smpc_get_timing(smpc_handle* h, float* ms4) {
    if (!h || !ms4) return SMPC_EINVAL;
    if (!h->timing) return fail(h, SMPC_ESTATE, "timing not enabled");
    if (!h->timed || !h->ev_complete[h->ev_cur]) return fail(h, SMPC_ESTATE, "no solve has been timed since smpc_enable_timing");
    (void)hipSetDevice(h->device);
    HIPCHK(h, hipEventSynchronize(h->ev_t[3]));
    // (the network pass comes first, ev0 -> ev1, then the stage builder -- linearisation + set-up in one kernel -- ev1 -> ev2)
    HIPCHK(h, hipEventElapsedTime(&ms4[1], h->ev_t[0], h->ev_t[1]));
    HIPCHK(h, hipEventElapsedTime(&ms4[0], h->ev_t[1], h->ev_t[2]));
    HIPCHK(h, hipEventElapsedTime(&ms4[2], h->ev_t[2], h->ev_t[3]));
    HIPCHK(h, hipEventElapsedTime(&ms4[3], h->ev_t[0], h->ev_t[3]));
    return SMPC_OK;
}

int smpc_get_qp_timing(smpc_handle* h, float* ms2) {
    if (!h || !ms2) return SMPC_EINVAL;
    if (!h->timing) return fail(h, SMPC_ESTATE, "timing not enabled");
    if (!h->timed || !h->ev_complete[h->ev_cur]) return fail(h, SMPC_ESTATE, "no solve has been timed since smpc_enable_timing");
    (void)hipSetDevice(h->device);
    HIPCHK(h, hipEventSynchronize(h->ev_t[3]));
    HIPCHK(h, hipEventElapsedTime(&ms2[0], h->ev_t[2], h->ev_t[4]));
    HIPCHK(h, hipEventElapsedTime(&ms2[1], h->ev_t[4], h->ev_t[3]));
    return SMPC_OK;
}

int smpc_get_timing_history(smpc_handle* h, int back, float* ms6) {
    if (!h || !ms6 || back < 0) return SMPC_EINVAL;
    for (int i = 0; i < 6; i++) ms6[i] = 0.0f;
    if (!h->timing || back >= smpc_handle::EV_RING || (long)back >= h->timed_count) return SMPC_OK;
    (void)hipSetDevice(h->device);
    const int slot = (h->ev_cur - back + 2 * smpc_handle::EV_RING) % smpc_handle::EV_RING;
    if (!h->ev_complete[slot]) return SMPC_OK;     // the solve that owns the slot returned early: valid stays 0
    hipEvent_t* ev = h->ev_sets[slot];
    if (hipEventQuery(ev[3]) != hipSuccess) { (void)hipGetLastError(); return SMPC_OK; }   // not finished yet: valid stays 0
    HIPCHK(h, hipEventElapsedTime(&ms6[1], ev[0], ev[1]));
    HIPCHK(h, hipEventElapsedTime(&ms6[0], ev[1], ev[2]));
    HIPCHK(h, hipEventElapsedTime(&ms6[2], ev[2], ev[4]));
    HIPCHK(h, hipEventElapsedTime(&ms6[3], ev[4], ev[3]));
    HIPCHK(h, hipEventElapsedTime(&ms6[4], ev[0], ev[3]));
    ms6[5] = 1.0f;
    return SMPC_OK;
}

int smpc_accumulate_stats(smpc_handle* h, int B, const int32_t* status, const int32_t* qp_iter, unsigned long long* acc3) {
    if (!h) return SMPC_EINVAL;
    if (B < 0 || !status || !acc3) return fail(h, SMPC_EINVAL, "bad argument");
    if (B == 0) return SMPC_OK;
    (void)hipSetDevice(h->device);
    hipLaunchKernelGGL(k_accumulate_stats, dim3((B + 63) / 64), dim3(64), 0, h->stream, B, status, qp_iter, acc3);
    HIPCHK(h, hipGetLastError());
    return SMPC_OK;
}

int smpc_get_qp_wave_stats(smpc_handle* h, double* out3) {
    if (!h || !out3) return SMPC_EINVAL;
    if (h->timing != 1 || !h->timed || !h->d_wstat.p) return fail(h, SMPC_ESTATE, "no solve has been timed since smpc_enable_timing(1)");
    (void)hipSetDevice(h->device);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    unsigned long long w[4];
    HIPCHK(h, hipMemcpy(w, h->d_wstat.p, sizeof(w), hipMemcpyDeviceToHost));
    const double tick_us = 1e-2;   // s_memrealtime: constant 100 MHz
    out3[0] = w[3] ? (double)w[0] / (double)w[3] * tick_us : 0.0;   // mean busy time of a half-wave (one instance), us
    out3[1] = w[3] ? (double)(w[2] - w[1]) * tick_us : 0.0;          // first start -> last end, us
    out3[2] = (double)w[3];
    return SMPC_OK;
}

}  // extern "C"

// Test hook (not part of include/smpc.h): what the scene slot and the context slot hold, copied to the host after the stream has
// drained -- tests/test_forecast_gpu.py holds smpc_forecast_scene's table against its numpy statement with it.  info[6] = {scene B,
// scene T, scene holds a forecast, context B, context T, context written by a forecast} (B = 0: the slot is empty); scene_out /
// ctx_out (either may be NULL) receive at most scene_cap doubles / ctx_cap floats.  Host pointers.
extern "C" int smpc_debug_scene_slots(smpc_handle* h, double* scene_out, size_t scene_cap, float* ctx_out, size_t ctx_cap, int64_t* info) {
    if (!h || !info) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t ns = (size_t)h->scene.B * (size_t)h->scene_T * h->desc.n_rows * SMPC_SCENE_ROW;
    const size_t nc = (size_t)h->ctx.B * (size_t)h->ctx_T * h->net->n_ctx;
    const int64_t inf[6] = {h->scene.B, h->scene_T, h->scene.B && h->scene_fc, h->ctx.B, h->ctx_T, h->ctx.B && h->ctx_fc};
    memcpy(info, inf, sizeof(inf));
    if (scene_out && ns) {
        if (ns > scene_cap) return fail(h, SMPC_EINVAL, "smpc_debug_scene_slots: the scene holds %zu doubles, room for %zu", ns, scene_cap);
        HIPCHK(h, hipMemcpy(scene_out, h->scene.d.p, ns * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (ctx_out && nc) {
        if (nc > ctx_cap) return fail(h, SMPC_EINVAL, "smpc_debug_scene_slots: the context holds %zu floats, room for %zu", nc, ctx_cap);
        HIPCHK(h, hipMemcpy(ctx_out, h->ctx.d.p, nc * sizeof(float), hipMemcpyDeviceToHost));
    }
    return SMPC_OK;
}

// Test hook (not part of include/smpc.h): the dispatch state a solve leaves behind, once the handle's stream has drained -- out[520] =
// [256] histogram of the solve's iteration counts (every instance of the launch adds itself once) | [256] bin cursors | the ticket of
// k_order_by_iters | the pair ticket of k_qp_ipm's crew | 6 unused.  Host pointer.
extern "C" int smpc_debug_qp_dispatch(smpc_handle* h, int32_t* out) {
    if (!h || !out) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    if (!h->d_ord_hist.p) return fail(h, SMPC_ESTATE, "smpc_debug_qp_dispatch: no solve yet");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, h->d_ord_hist.p, 520 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SMPC_OK;
}

// Test hook (not part of include/smpc.h): the stage records of the QP workspace as the solve path builds them (path 1: MLP ->
// k_stage_build) or as the thread-per-node kernels of rounds 1-3 do (path 0: k_node_linearise -> MLP -> k_qp_setup, off the solve
// path and kept as this independent reference), copied to the host, and the layout's offsets -- so that tests/test_gpu_parity.py
// can compare the two builders block by block.  Host pointers.  layout[24] = {stride, nIMG, oIMG, oSL, nF, oR0, oR1, oR2, oCZA,
// oCZN, oZ, oZN, NRT, nJ, doubles per instance, record version, iTT, iGT, iGN, iB, iSC, iHQQ, iGZ, 0}.
extern "C" int smpc_debug_stage_records(smpc_handle* h, int B, const double* x0, const double* xg, const double* ug, const double* p,
                                        int path, double* ws_out, int32_t* layout) {
    if (!h || B <= 0 || !x0 || !xg || !ug || !p || !ws_out || !layout) return SMPC_EINVAL;
    (void)hipSetDevice(h->device);
    int rc;
    if ((rc = guard_solve_slots(h, B, "smpc_debug_stage_records"))) return rc;
    if ((rc = ensure_batch(h, B))) return rc;
    const int N = h->N, nx = 2 * h->desc.nq, nu = h->desc.nq;
    Stage io{h, false};
    const double *dx0, *dxg, *dug, *dp;
    if ((rc = io.place([&](Stage& v) {
             dx0 = v.in(x0, (size_t)B * nx);
             dxg = v.in(xg, (size_t)B * (N + 1) * nx);
             dug = v.in(ug, (size_t)B * N * nu);
             dp = v.in(p, (size_t)B * (N + 1) * SMPC_NP);
         })))
        return rc;
    const size_t per = ws_doubles_per_instance(h, N);
    HIPCHK(h, hipMemsetAsync(h->d_ws.p, 0, per * (size_t)B * sizeof(double), h->stream));
    // The two builders of every nq, named outside any template: a kernel's place in the code object (see ensure_batch) follows the
    // first such mention -- what a generic lambda names counts only once it is instantiated, depth first, at the end of the file.
    // These keep k_stage_build and k_qp_setup behind every other kernel, one nq after the other; without them launch_solve's own
    // call would put k_stage_build ahead of k_qp_ipm_wg.
    (void)&launch_stage_records<5>, (void)&launch_stage_records_per_node<5>;
    (void)&launch_stage_records<6>, (void)&launch_stage_records_per_node<6>;
    (void)&launch_stage_records<7>, (void)&launch_stage_records_per_node<7>;
    if ((rc = with_nq(h, [&](auto NQ) {
             return path == 1 ? launch_stage_records<NQ>(h, B, dx0, dxg, dug, dp, false) : launch_stage_records_per_node<NQ>(h, B, dx0, dxg, dug, dp);
         })))
        return rc;
    HIPCHK(h, hipMemcpyAsync(ws_out, h->d_ws.p, per * (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if ((rc = io.finish())) return rc;
    return with_nq(h, [&](auto NQ) {
        const QpLayout<NQ> Ly(h->desc.n_rows);
        const int v[24] = {Ly.stride, Ly.nIMG, Ly.oIMG, Ly.oSL, Ly.nF, Ly.oR0, Ly.oR1, Ly.oR2, Ly.oCZA, Ly.oCZN, Ly.oZ, Ly.oZN, Ly.NRT, Ly.nJ,
                           (int)per, 12, Ly.iTT, Ly.iGT, Ly.iGN, Ly.iB, Ly.iSC, Ly.iHQQ, Ly.iGZ, 0};
        for (int i = 0; i < 24; i++) layout[i] = v[i];
        return SMPC_OK;
    });
}

#ifdef QP_PROFILE
// diagnostic builds only (not part of include/smpc.h): per-phase shader-clock sums of k_qp_ipm since the last call
extern "C" int smpc_debug_qp_profile(unsigned long long* out16) {
    unsigned long long zero[16] = {0};
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(smpc::g_qp_prof), sizeof(zero)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(smpc::g_qp_prof), zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
extern "C" int smpc_debug_qp_wg_profile(unsigned long long* out16) {
    unsigned long long zero[16] = {0};
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(smpc::g_wg_prof), sizeof(zero)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(smpc::g_wg_prof), zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
#endif
