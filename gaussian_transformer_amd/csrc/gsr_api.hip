// gsr_api.hip -- the entry points of include/gsr.h: argument validation, workspace carving, options (one snapshot per call), the plan both
// passes share, stage sequencing on the caller's stream, and the library's one error path (gsr_host.h: fail() and the buffer of gsr_last_error()).
// Host code only.  The entry points of every other header (gsr_loss.h, gsr_optim.h, gsr_density.h, gsr_knn.h, gsr_chamfer.h,
// gsr_sequence.h, gsr_rows.h) live in the translation unit that holds their kernels.
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>

#include "../../include/gsr.h"
#include "gsr_host.h"
#include "gsr_internal.h"

namespace gsr {

static thread_local char g_err[GSR_ERR_TEXT_BYTES] = "";
// process-wide (not thread-local): PyTorch's autograd engine calls gsr_backward from its own thread
static std::atomic<int> g_profiling{0};
static std::atomic<int> g_exact_cull{1};       // output-invariant exact splat-vs-tile culling
static std::atomic<int> g_bwd_npx{2};          // 8x8 pixel blocks per wave in the reverse compositing kernel (1, 2 or 4)
static std::atomic<int> g_fwd_npx{2};          // same for the forward compositing kernel
static std::atomic<int> g_wpb{1};              // waves per workgroup of the compositing kernels (waves are independent)
static std::atomic<int> g_two_level_sort{1};   // 1: depth order first, then per-tile lists; 0: one global sort on tile<<32|depth
static std::atomic<int> g_tile_lists{2};       // 2: supertile_sort.hip (per-super-tile LDS order, no global sort); 1: depth_order.hip + tile_lists.hip
                                               // (round 1's path, also the fall-back of 2); 0: key emission + rocPRIM sort + range detection
static std::atomic<int> g_depth_buckets{1};    // 0: rocPRIM radix sort + scan; 1: depth_order.hip when P is large enough; 2: always (tests)
int g_composite_lds_pad = 0;                    // debug: extra dynamic LDS bytes per compositing workgroup (occupancy experiments)
static std::atomic<int> g_count_lanes{0};      // 1: instrumented compositing kernels (lane-slot accounting, slower)
static std::atomic<int> g_deterministic_bwd{0};   // 1: fixed-order reduction of the reverse pass's partial gradients
static std::atomic<int> g_seg_len{256};           // entries per segment of the reverse pass's work units (multiple of 64); 0: whole half tiles
static std::atomic<int> g_dense_pergauss{2};      // per-Gaussian backward on the Gaussians with a gradient only, zero rows filled on a second stream: 0 off, 1 on, 2 = from GSR_DENSE_MIN_P Gaussians
static std::atomic<int> g_prefill_at{1};           // announced gradient outputs (gsr_backward_prefill): zero-filled 1 = beside the forward compositing kernel, 2 = beside the list-ordering kernel already, 0 = announcements ignored
static std::atomic<int> g_dense_fork{2};           // dense per-Gaussian stage: 1 = the second stream is forked after the accumulator rows are cleared, 0 = before, 2 = after below GSR_DENSE_FORK_EARLY_P Gaussians
static std::atomic<int> g_fwd_pair_long{-1};       // forward pass on small images (make_plan: persistent reverse kernel in use): half tiles whose list exceeds this many entries are walked by two waves, one per block; 0 = off, -1 = GSR_PAIR_LONG_DEFAULT
static std::atomic<int> g_bwd_lpt{1};             // large images: the reverse pass's half tiles in order of decreasing length (composite_bwd_lpt_kernel); 0 = in tile order
static std::atomic<int> g_asm_walk{1};            // 1: compositing walks written in gfx950 assembly where they exist (same results, bit for bit), 0: the C++ walks
static std::atomic<int> g_fill_in_tail{0};        // 1: with the persistent reverse kernel, the zero rows of Gaussians without a gradient are written by its idle waves
                                                  // (measured at config 3: pergauss_bwd 84 -> 62 us, but the compositing kernel + 40..66 us: off)
static std::atomic<int> g_persistent_bwd{2};      // persistent reverse compositing kernel drawing length-ordered work units (2 blocks per wave only): 0 never, 1 always,
                                                  // 2 (default) when the image has at most GSR_PERSISTENT_MAX_TILES tiles, i.e. when its half tiles fill the chip less
                                                  // than 1.5 times over and the longest chain, not the throughput, sets the kernel's time (measured: -25 % at 800 x 800,
                                                  // -10 % at 1600 x 900, +-0 at 1080p and 4K where the classic kernel's second generation of waves hides the long chains)
#define GSR_PERSISTENT_MAX_TILES 6144
#define GSR_DEPTH_BUCKETS_MIN_P 1024           // measured at P = 10 k: 25 us against 48 us for rocPRIM sort + scan + copy-back

// State that adapts to what a device has rendered lives per DEVICE, not per process: a frame with depth outliers on one
// GPU must not change the path of another GPU driven by the same process (SURVEY 8b "several devices in one process").
// The knobs above are deliberate process-wide settings (gsr_set_option); everything below is keyed by hipGetDevice().
#define GSR_MAX_DEVICES 32
struct DeviceState {
    std::atomic<int> bucket_fail_p{0x7fffffff};   // smallest P whose buckets overflowed even under the log map: not tried again
    std::atomic<int> depth_log_map{0};            // set once a frame overflowed a depth bucket under the linear map: log map from then on
    std::atomic<int> poll_timeouts{0};            // N read-backs whose pinned-word poll timed out (diagnostic)
    std::atomic<uint32_t> frame_seq{0};           // forward passes so far: the mark composite_fwd leaves in GeomView::touched cycles with it
    std::mutex mu;                                // guards stage_ms and counters
    float stage_ms[GSR_NUM_STAGES] = {0};         // last profiled forward / backward on this device
    CompositeCounters *counters = nullptr;        // [2] device memory: forward, reverse (allocated on first use of count_lanes)
    // gsr_backward's second stream (lowest priority): the zero-fill of the gradient outputs runs there, beside the compositing kernel
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_prefill = nullptr;
    bool side_failed = false;
    // gsr_backward_prefill: the outputs announced for the backward call that follows the next forward pass (pending), and the ones
    // that forward pass zero-filled (done; single use, dropped by the next gsr_forward or gsr_backward on the device)
    struct Prefill { bool pending = false, done = false; int P = 0, M = 0; float *p[9] = {nullptr}; } prefill;
};
static DeviceState g_dev[GSR_MAX_DEVICES];
static DeviceState &dev_state() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0) d = 0;
    return g_dev[d % GSR_MAX_DEVICES];
}
// device buffer of the instrumented compositing kernels (debug facility: the only allocation the library makes besides
// its pinned read-back words); NULL when counting is off (count_lanes: the call's Options) or the allocation failed
static CompositeCounters *lane_counters(DeviceState &ds, int count_lanes, int which) {
    if (!count_lanes) return nullptr;
    std::lock_guard<std::mutex> lk(ds.mu);
    if (!ds.counters) {
        // two counter blocks, then two per-unit trace arrays (wave timeline of the instrumented kernels)
        const size_t tr_bytes = (size_t)GSR_TRACE_UNITS * sizeof(uint4);
        if (hipMalloc((void **)&ds.counters, 2 * sizeof(CompositeCounters) + 2 * tr_bytes) != hipSuccess) { ds.counters = nullptr; return nullptr; }
        (void)hipMemset(ds.counters, 0, 2 * sizeof(CompositeCounters) + 2 * tr_bytes);
        CompositeCounters h[2];
        memset(h, 0, sizeof(h));
        for (int w = 0; w < 2; w++) {
            h[w].trace = reinterpret_cast<uint4 *>(reinterpret_cast<char *>(ds.counters + 2) + (size_t)w * tr_bytes);
            h[w].trace_cap = GSR_TRACE_UNITS;
        }
        (void)hipMemcpy(ds.counters, h, sizeof(h), hipMemcpyHostToDevice);
    }
    return ds.counters + which;
}
// the device's second stream and its two events, made on first use (false: could not be made -- the caller keeps everything on one stream)
static bool side_stream(DeviceState &ds) {
    if (ds.side) return true;
    if (ds.side_failed) return false;
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (hipStreamCreateWithPriority(&ds.side, hipStreamNonBlocking, least) != hipSuccess ||
        hipEventCreateWithFlags(&ds.ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ds.ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ds.ev_prefill, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        ds.side = nullptr; ds.side_failed = true;
        return false;
    }
    return true;
}
// ---- gsr_forward's side of gsr_backward_prefill: take the announcement, fork the fill, publish it as done.  The zeros of the announced
// gradient outputs are written on the device's second stream beside the forward pass's last kernels (half of the CUs idle under the
// list-ordering kernel, most of them in the compositing kernel's tail) instead of beside the reverse compositing kernel, whose waves leave
// no slot free until it drains.  The call's copy `pre` uses the flags for itself: pending = to be filled by this call, done = filled. ----
// joins an earlier render's fill that no gsr_backward took over; pre->pending = announced for this (P, M), `wanted`, and there is a second stream
static int32_t prefill_take(DeviceState &ds, hipStream_t s, bool wanted, int P, int M, DeviceState::Prefill *pre) {
    std::lock_guard<std::mutex> lk(ds.mu);
    if (ds.prefill.done) {
        ds.prefill.done = false;
        if (hipStreamWaitEvent(s, ds.ev_prefill, 0) != hipSuccess) return fail(GSR_ERR_HIP, "prefill join");
    }
    if (!ds.prefill.pending) return GSR_OK;
    ds.prefill.pending = false;
    *pre = ds.prefill;
    pre->pending = wanted && pre->P == P && pre->M == M && pre->p[5] && !pre->p[6] && side_stream(ds);
    return GSR_OK;
}
static int32_t prefill_fork(DeviceState &ds, hipStream_t s, const float *shs, DeviceState::Prefill *pre) {      // at most once per call
    if (!pre->pending) return GSR_OK;
    pre->pending = false;
    std::lock_guard<std::mutex> lk(ds.mu);
    PergaussBwdArgs fa{};
    fa.P = pre->P; fa.M = pre->M; fa.shs = shs; fa.dL_dmeans2D = pre->p[0]; fa.dL_dopacity = pre->p[1]; fa.dL_dcolors = pre->p[2];
    fa.dL_dmeans3D = pre->p[3]; fa.dL_dcov3D = pre->p[4]; fa.dL_dsh = pre->p[5]; fa.dL_dscales = pre->p[7]; fa.dL_drots = pre->p[8];
    HIP_TRY(hipEventRecord(ds.ev_fork, s), "prefill fork event");
    HIP_TRY(hipStreamWaitEvent(ds.side, ds.ev_fork, 0), "prefill fork wait");
    HIP_TRY(launch_fill_zero(fa, ds.side), "gradient zero-fill launch");
    HIP_TRY(hipEventRecord(ds.ev_prefill, ds.side), "prefill event");
    pre->done = true;
    return GSR_OK;
}
// joined by the gsr_backward that takes the buffers over, or by the next call on the device (the fill's tail runs on between the passes)
static void prefill_publish(DeviceState &ds, const DeviceState::Prefill &pre) {
    if (!pre.done) return;
    std::lock_guard<std::mutex> lk(ds.mu);
    ds.prefill = pre;
}
#define GSR_PAIR_LONG_DEFAULT 64
#define GSR_LPT_SPAN 512              // length classes of the reverse pass's order on large images: 16 of 32 entries (SegView, plan_units)
#define GSR_DENSE_MIN_P 500000
#define GSR_DENSE_FORK_EARLY_P 2000000

// One call's view of the options: gsr_forward, gsr_backward and gsr_backward_workspace_bytes make one at their top, which reads every atomic
// once, and decide everything from it, so that a gsr_set_option from another thread cannot give one call two answers.
struct Options {
    const int profiling = g_profiling.load(), exact_cull = g_exact_cull.load(), bwd_npx = g_bwd_npx.load(), fwd_npx = g_fwd_npx.load(), wpb = g_wpb.load(),
              two_level_sort = g_two_level_sort.load(), tile_lists = g_tile_lists.load(), depth_buckets = g_depth_buckets.load(),
              count_lanes = g_count_lanes.load(), deterministic_bwd = g_deterministic_bwd.load(), seg_len = g_seg_len.load(),
              dense_pergauss = g_dense_pergauss.load(), prefill_at = g_prefill_at.load(), dense_fork = g_dense_fork.load(), fwd_pair_long = g_fwd_pair_long.load(),
              bwd_lpt = g_bwd_lpt.load(), asm_walk = g_asm_walk.load(), fill_in_tail = g_fill_in_tail.load(), persistent_bwd = g_persistent_bwd.load();
};

// What gsr_forward and gsr_backward must agree on, decided in this one place from the options, P and the image size alone: the forward
// pass leaves checkpoints, half-tile lengths and zero-filled outputs only where the reverse pass of the same (options, P, W, H) uses them.
// Each pass adds what only it can know (R > 0, deterministic buffers, lane counters, pointers, workspace sizes).  Where their rules differ, each keeps its own:
//   - length order: the forward pass files the lengths under `lpt_span && seg_len == 0 && T <= 1 << 28`, the reverse pass reads them under
//     `lpt_span && !persistent` (+ its own conjuncts, no bound on T).  seg_len == 0 is not !persistent_bwd: with deterministic_bwd or
//     segment_entries 0 under persistent_bwd 1, a large image's forward pass files lengths that the persistent kernel never reads
//   - dense stage: the forward pass prefills under `dense_wanted` and a short test of its own (SH colours in one tensor of M == 16,
//     scales and rotations, dL_dsh announced without dL_dsh_rest), the reverse pass asks pergauss_dense_eligible()
struct Plan {
    int gridx, gridy, T;      // tiles; T as the forward pass has always computed it (int)
    bool small_image;         // at most GSR_PERSISTENT_MAX_TILES tiles: the longest chain, not the throughput, sets the compositing kernels' time
    bool persistent_bwd;      // the reverse compositing kernel is the persistent one (gsr_backward: and R > 0)
    int seg_len;              // > 0: the forward pass takes checkpoints every seg_len entries and leaves the half tiles' lengths for that kernel
    int pair_long_n;          // > 0: the forward pass walks half tiles with more entries than this by two waves, one per block
    int lpt_span;             // > 0: image and options allow the reverse pass's half tiles in order of decreasing length (composite_bwd_lpt_kernel)
    bool dense_wanted;        // dense_pergauss says the per-Gaussian stage runs on the Gaussians with a gradient only
};
static Plan make_plan(const Options &o, int P, int W, int H) {
    Plan p;
    p.gridx = grid_dim(W); p.gridy = grid_dim(H);
    const long long T = (long long)p.gridx * p.gridy;
    p.T = (int)T; p.small_image = T <= GSR_PERSISTENT_MAX_TILES;
    const bool pk = (o.persistent_bwd == 1 || (o.persistent_bwd == 2 && p.small_image)) && T <= (1 << 28);
    p.persistent_bwd = pk && o.bwd_npx == 2;
    // not under deterministic_bwd: which half tiles get checkpoints once the pool runs out is a race between the forward waves, and a
    // segment that starts from a stored transmittance differs in the last bits from the same entries reached by dividing back
    p.seg_len = pk && o.fwd_npx == 2 && !o.deterministic_bwd ? o.seg_len : 0;
    // long lists by pairs of block waves: only where the longest list sets the kernel's time (the images the persistent reverse kernel serves)
    p.pair_long_n = p.small_image && o.fwd_npx == 2 ? (o.fwd_pair_long < 0 ? GSR_PAIR_LONG_DEFAULT : o.fwd_pair_long) : 0;
    p.lpt_span = !p.small_image && o.bwd_lpt && o.fwd_npx == 2 && o.bwd_npx == 2 ? GSR_LPT_SPAN : 0;
    p.dense_wanted = o.dense_pergauss == 1 || (o.dense_pergauss == 2 && P >= GSR_DENSE_MIN_P);
    return p;
}
static const char *const k_stage_names[GSR_NUM_STAGES] = {
    // lists.bin = entries binned per super-tile (count + scan + scatter; round 1's path: depth order + scan); lists.order = per-super-tile order +
    // expansion into the tile lists (sort path: the radix sort); emit_keys / ranges only run on the sort path
    "fwd.preprocess", "fwd.lists.bin", "fwd.readback_N", "fwd.lists.emit_keys", "fwd.lists.order", "fwd.lists.ranges", "(unused)",
    "fwd.composite", "bwd.clear+plan", "bwd.composite", "bwd.pergauss", "fwd.total", "bwd.total"};

int fail(int code, const char *fmt, ...) {      // gsr_host.h: every entry point of every translation unit reports through this
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
static int32_t hip_rc(hipError_t e, const char *what) { HIP_TRY(e, what); return GSR_OK; }      // the last HIP call of a function

GeomView carve_geom(void *base, int P, size_t scan_tb, size_t dsort_tb) {
    GeomView g;
    const size_t n = (size_t)(P > 0 ? P : 1);
    Bump w = {(char *)base, 0};
    g.rec = w.take<float>(n * GSR_REC_FLOATS); g.depth = w.take<float>(n); g.opac = w.take<float>(n);
    g.rect = w.take<uint4>(n); g.tiles = w.take<uint32_t>(n); g.offsets = w.take<uint32_t>(n); g.clamped = w.take<uint8_t>(n);
    g.perm = w.take<uint32_t>(n); g.depth_sorted = w.take<uint32_t>(n); g.orect = w.take<uint4>(n);
    g.ss_rec = w.take<uint4>(n); g.hot = w.take<uint32_t>(n); g.ss_entries = w.take<uint4>((size_t)GSR_SS_ENT_PER_G * n);
    // the bin count is an image property the workspace size cannot depend on (gsr_workspace_sizes is asked per (P, W, H) but
    // carve_geom only sees P): room for GSR_SS_WGCNT_WORDS words; supertile_sort.hip is skipped when nblk * S exceeds it
    g.ss_wg_cnt = w.take<uint32_t>(GSR_SS_WGCNT_WORDS);
    g.tl_mat1 = w.take<uint32_t>((size_t)GSR_TL_MAX_S * ((n + GSR_TL_L1 - 1) / GSR_TL_L1)); g.tl_bin_total = w.take<uint32_t>(GSR_TL_MAX_S);
    g.scan_temp = w.take<char>(scan_tb); g.scan_temp_bytes = scan_tb;
    g.dsort_temp = w.take<char>(dsort_tb); g.dsort_temp_bytes = dsort_tb;
    const size_t npre = (size_t)depth_order_plan(P, 0).npre;   // the bucket tables are sized for the maximum
    g.dord.hdr = w.take<uint32_t>(GSR_DO_ZERO_WORDS);
    g.dord.gpair = reinterpret_cast<unsigned long long *>(g.dord.hdr + DO_HDR_WORDS);     // DO_HDR_WORDS is even: 8-byte aligned
    g.dord.gcur = g.dord.hdr + DO_HDR_WORDS + 2 * GSR_DO_MAXB;
    g.dord.bstart = w.take<uint32_t>(GSR_DO_MAXB + 1); g.dord.tbase = w.take<uint32_t>(GSR_DO_MAXB + 1);
    g.dord.blkmin = w.take<uint32_t>(npre); g.dord.blkmax = w.take<uint32_t>(npre); g.dord.blkent = w.take<uint32_t>(npre);
    g.dord.comp = w.take<uint64_t>(n); g.touched = w.take<uint8_t>(n); g.touch_mark = w.take<uint32_t>(1);
    g.total_bytes = w.off;
    return g;
}
int32_t view_geom(const void *ws, size_t bytes, int P, GeomView *g) {
    size_t stb = 0, dtb = 0;
    HIP_TRY(scan_temp_bytes(P, &stb), "scan temp query");
    HIP_TRY(depth_sort_temp_bytes(P, &dtb), "depth sort temp query");
    *g = carve_geom(const_cast<void *>(ws), P, stb, dtb);
    return bytes < g->total_bytes ? fail(GSR_ERR_WORKSPACE, "geom workspace %zu < %zu", bytes, g->total_bytes) : GSR_OK;
}

ImageView carve_image(void *base, int W, int H) {
    ImageView v;
    const size_t T = (size_t)((W + GSR_TILE_HOST - 1) / GSR_TILE_HOST) * ((H + GSR_TILE_HOST - 1) / GSR_TILE_HOST);
    const size_t HW = (size_t)W * H;
    Bump w = {(char *)base, 0};
    v.ranges = w.take<uint2>(T > 0 ? T : 1); v.final_T = w.take<float>(HW > 0 ? HW : 1); v.n_contrib = w.take<uint32_t>(HW > 0 ? HW : 1);
    const size_t units = 2 * (T > 0 ? T : 1);
    v.seg.units = (uint32_t)units; v.seg.band_units = (uint32_t)((units + GSR_SEG_BANDS - 1) / GSR_SEG_BANDS);
    v.seg.pool_cap = (uint32_t)((units * GSR_SEG_POOL_PER_UNIT + GSR_SEG_BANDS - 1) / GSR_SEG_BANDS * GSR_SEG_BANDS);
    v.seg.hdr = w.take<uint32_t>(GSR_SEG_HDR_WORDS); v.seg.info = w.take<uint2>(units); v.seg.ck_slot = w.take<uint32_t>(units * 8);
    v.seg.list_cap = (uint32_t)((size_t)v.seg.band_units * (1 + GSR_SEG_MAXCK) + GSR_SEG_FILL_CAP);
    v.seg.bq = w.take<uint4>((size_t)GSR_SEG_BANDS * v.seg.list_cap); v.seg.pool = w.take<float4>((size_t)v.seg.pool_cap * 128);
    v.total_bytes = w.off;
    return v;
}
int32_t view_image(const void *ws, size_t bytes, int W, int H, ImageView *im) {
    *im = carve_image(const_cast<void *>(ws), W, H);
    return bytes < im->total_bytes ? fail(GSR_ERR_WORKSPACE, "image workspace %zu < %zu", bytes, im->total_bytes) : GSR_OK;
}

BinningView carve_binning(void *base, int64_t N, size_t sort_tb) {
    BinningView b;
    const size_t n = (size_t)(N > 0 ? N : 1);
    Bump w = {(char *)base, 0};
    b.point_list = w.take<uint32_t>(n); b.contrib = w.take<uint8_t>(4 * n);
    b.list_bytes = w.off;
    b.keys_sorted = w.take<uint64_t>(n); b.keys_unsorted = w.take<uint64_t>(n); b.point_list_unsorted = w.take<uint32_t>(n);
    b.tkeys_unsorted = (uint32_t *)b.keys_sorted; b.ids_sorted = b.point_list; b.ids_unsorted = (uint32_t *)b.keys_unsorted;
    b.tkeys_sorted = b.point_list_unsorted;
    b.sort_temp = w.take<char>(sort_tb); b.sort_temp_bytes = sort_tb;
    b.total_bytes = w.off;
    return b;
}
int32_t view_lists(const void *ws, size_t bytes, int64_t R, BinningView *b) {
    *b = carve_binning(const_cast<void *>(ws), R, 0);
    return R > 0 && bytes < b->list_bytes ? fail(GSR_ERR_WORKSPACE, "binning workspace too small for R=%lld (%zu < %zu)", (long long)R, bytes, b->list_bytes) : GSR_OK;
}

BackwardView carve_backward(void *ws, int P, size_t det_bytes) {
    BackwardView v;
    Bump w = {(char *)ws, 0};
    const size_t acc_floats = acc_rows(P) * GSR_ACC_FLOATS;
    v.acc = w.take<float>(acc_floats); v.acc_bytes = acc_floats * sizeof(float);
    v.det_end = w.off + det_bytes; v.det = det_bytes ? (float *)w.take<char>(det_bytes) : nullptr;
    v.vis_off = w.off; v.vis_cap = pergauss_vis_cap(P);
    v.vis_count = w.take<uint32_t>(1); v.vis_list = w.take<uint32_t>((size_t)P);      // the counter on a line of its own
    v.vis_rec = w.take_last<float4>((size_t)v.vis_cap * 15);                           // [vis_cap / 64][15][64]
    v.total_bytes = w.off;
    return v;
}

TileListView carve_tile_lists(void *base, const TileListPlan &pl, int64_t E) {
    TileListView v;
    Bump w = {(char *)base, 0};
    const size_t S = (size_t)pl.S, e = (size_t)(E > 0 ? E : 1), nseg = (size_t)(pl.nseg_max > 0 ? pl.nseg_max : 1);
    v.binstart = w.take<uint32_t>(S + 1); v.segbase = w.take<uint32_t>(S + 1);
    v.seg_super = w.take<uint32_t>(nseg); v.entries = w.take<uint4>(e); v.segcnt = w.take<uint32_t>(nseg * 64);
    v.tile_off = w.take<uint32_t>(S * 64); v.tile_tot = w.take<uint32_t>(S * 64); v.st_pairs = w.take<uint32_t>(S);
    v.total_bytes = w.off;
    return v;
}

static inline int tile_bits(int W, int H) { return ceil_log2_u32((uint32_t)(grid_dim(W) * grid_dim(H))); }
static inline int key_bits(int W, int H) { return 32 + tile_bits(W, H); }
// temp storage that serves either sort flavour
static hipError_t any_sort_temp_bytes(int64_t N, int W, int H, size_t *bytes) {
    size_t a = 0, b = 0;
    hipError_t e = sort_temp_bytes(N, key_bits(W, H), &a);
    if (e != hipSuccess) return e;
    e = sort2_temp_bytes(N, tile_bits(W, H) > 0 ? tile_bits(W, H) : 1, &b);
    *bytes = a > b ? a : b;
    return e;
}

// Four pinned host words per in-flight forward call: the bucket-scan kernel stores {overflow, Pv, N, seq}
// into them and the host polls `seq`, so nothing (copy engine, barrier packet) sits between the kernels that
// produce the totals and the kernels queued behind them while the host catches up.
struct ReadbackSlot {
    std::atomic<int> busy{0};
    uint32_t *host = nullptr;     // 8 pinned, device-visible words: overflow, Pv, N, E, seq
    int device = -1;
};
static ReadbackSlot g_slots[8];
static std::atomic<uint32_t> g_seq{1};
static ReadbackSlot *acquire_slot() {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    for (auto &sl : g_slots) {
        int expect = 0;
        if (!sl.busy.compare_exchange_strong(expect, 1)) continue;
        if (sl.host && sl.device != dev) { sl.busy.store(0); continue; }
        if (!sl.host) {
            // coherent + mapped: the kernel's system-scope store must become visible to the polling host while the
            // stream is still running, whatever HIP_HOST_COHERENT says
            if (hipHostMalloc((void **)&sl.host, 8 * sizeof(uint32_t), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) { sl.host = nullptr; sl.busy.store(0); return nullptr; }
            sl.device = dev;
        }
        return &sl;
    }
    return nullptr;
}
static void release_slot(ReadbackSlot *sl) { if (sl) sl->busy.store(0); }
// spin on the sequence word; gives up after ~2 s (the caller then synchronises the stream instead, counts the
// time-out in the device's "poll_timeouts" and reuses the slot: after the synchronisation nothing writes to it)
static bool wait_seq(const ReadbackSlot *sl, uint32_t seq) {
    timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (uint32_t spin = 1;; spin++) {
        if (__atomic_load_n(&sl->host[4], __ATOMIC_ACQUIRE) == seq) return true;
        __builtin_ia32_pause();
        if ((spin & 0xfffffu) == 0) {
            clock_gettime(CLOCK_MONOTONIC, &t1);
            if (t1.tv_sec - t0.tv_sec > 2) return false;
        }
    }
}

struct StageTimer {   // hipEvent pairs on the caller's stream; active only under gsr_set_profiling(1)
    hipStream_t s;
    bool on;
    hipEvent_t ev[GSR_NUM_STAGES + 1];
    int idx[GSR_NUM_STAGES + 1];
    float ms_out[GSR_NUM_STAGES];
    int n = 0;
    DeviceState &ds;           // where finish() files the times
    StageTimer(hipStream_t s_, bool on_, DeviceState &ds_) : s(s_), on(on_), ds(ds_) { for (float &m : ms_out) m = -1.f; }
    void zero(int stage) { ms_out[stage] = 0.f; }
    void mark(int stage_about_to_start) {
        if (!on || n > GSR_NUM_STAGES) return;
        if (hipEventCreate(&ev[n]) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(ev[n], s);
        idx[n] = stage_about_to_start;
        n++;
    }
    void finish(int total_slot) {   // call after a final mark(-1)
        if (!on || n < 2) return;
        (void)hipEventSynchronize(ev[n - 1]);
        for (int i = 0; i + 1 < n; i++) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            if (idx[i] >= 0) ms_out[idx[i]] = ms;
        }
        float tot = 0.f;
        (void)hipEventElapsedTime(&tot, ev[0], ev[n - 1]);
        ms_out[total_slot] = tot;
        {
            std::lock_guard<std::mutex> lk(ds.mu);
            for (int i = 0; i < GSR_NUM_STAGES; i++) if (ms_out[i] >= 0.f) ds.stage_ms[i] = ms_out[i];
        }
        for (int i = 0; i < n; i++) (void)hipEventDestroy(ev[i]);
        n = 0;
    }
};

// One gsr_forward or gsr_backward call: what its stages share.  The device state is looked up, the options are read and the plan is
// made once, here; the views are taken (view_geom, view_image) once the arguments have passed their checks.
struct Call {
    hipStream_t s;
    int P, W, H, debug;
    DeviceState &ds;
    const Options o;
    const Plan pl;
    StageTimer tm;
    GeomView g; ImageView im;                // view_geom, view_image
    // gsr_forward only: the caller's allocator for the binning workspace with its argument, and where it wants N (may be NULL)
    gsr_alloc_fn alloc = nullptr; void *alloc_user = nullptr; int64_t *num_rendered = nullptr;
    DeviceState::Prefill pre;                // the announcement this render fills (prefill_take)
    uint32_t touch_mark = 0;                 // this frame's mark for GeomView::touched
    bool lists_done = false, tile_lists = false;   // the super-tile builder has made the lists; else: tile_lists.hip makes them (fwd_depth_order)
    BinningView b;                           // the lists, once a builder has allocated them
    int P_list = 0;                          // entries of the depth-ordered list (perm / offsets)
    int64_t N = 0, E = 0;                    // (Gaussian, tile) pairs and (Gaussian, super-tile) entries of this frame
    Call(gsr_stream_t stream, int P_, int W_, int H_, int debug_)
        : s((hipStream_t)stream), P(P_), W(W_), H(H_), debug(debug_), ds(dev_state()), pl(make_plan(o, P_, W_, H_)),
          tm(s, o.profiling != 0, ds) {}
};

// Reads back the four totals {overflow, Pv or largest bin, N, E} of the kernels `launch(host_out, seq)` queues: they store them into a
// pinned slot and the host polls its sequence word, so that neither a copy nor a barrier sits between those kernels and the ones queued
// behind them.  Without a slot (none free, or debug mode) or when the poll times out, the words are copied from the workspace header (the first
// from [DO_OVERFLOW], the other three from `rest`; NULL: they follow the first) and the stream is synchronised.  Every path releases the slot.
template <class Launch>
static int32_t read_totals(Call &c, const char *what, Launch launch, const uint32_t *rest, uint32_t h[4]) {
    ReadbackSlot *sl = c.debug ? nullptr : acquire_slot();
    const uint32_t seq = sl ? (g_seq.fetch_add(1) | 0x80000000u) : 0u;
    if (sl) sl->host[4] = 0u;
    const hipError_t e = launch(sl ? sl->host : nullptr, seq);
    if (e != hipSuccess) { release_slot(sl); return fail(GSR_ERR_HIP, "%s: %s (%d)", what, hipGetErrorString(e), (int)e); }
    if (c.debug) HIP_TRY(hipStreamSynchronize(c.s), what);
    c.tm.mark(2);
    if (sl && wait_seq(sl, seq)) { h[0] = sl->host[0]; h[1] = sl->host[1]; h[2] = sl->host[2]; h[3] = sl->host[3]; release_slot(sl); return GSR_OK; }
    hipError_t ce = hipMemcpyAsync(h, c.g.dord.hdr + DO_OVERFLOW, (rest ? 1 : 4) * sizeof(uint32_t), hipMemcpyDeviceToHost, c.s);
    if (ce == hipSuccess && rest) ce = hipMemcpyAsync(h + 1, rest, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, c.s);
    if (ce == hipSuccess) ce = hipStreamSynchronize(c.s);
    if (sl) { c.ds.poll_timeouts.fetch_add(1); release_slot(sl); }      // the stream has drained: the kernel that writes the slot has finished, so it is free again
    return ce == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "read N: %s (%d)", hipGetErrorString(ce), (int)ce);
}

// ---- gsr_forward's stages (the checks let P == 0 pass after the first two: gsr_forward then only clears the image) ----
static int32_t fwd_check(const PreprocessArgs &a, const float *bg, const float *out_color, const void *geom_ws, const void *img_ws, gsr_alloc_fn alloc) {
    if (a.P < 0 || a.W <= 0 || a.H <= 0 || !out_color || !bg || !a.viewmatrix || !a.projmatrix) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_forward: bad sizes or missing bg/matrices/out_color");
    if (a.W > 65535 * GSR_TILE_HOST || a.H > 65535 * GSR_TILE_HOST) return fail(GSR_ERR_INVALID_ARGUMENT, "image too large");
    if (a.P == 0) return GSR_OK;
    if (!a.means3D || !a.opacities || !a.radii || !geom_ws || !img_ws || !alloc) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_forward: missing means3D/opacities/radii/workspaces/allocator");
    if ((a.shs != nullptr) == (a.colors_precomp != nullptr)) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_forward: exactly one of shs / colors_precomp must be given");
    if (((a.scales != nullptr) && (a.rotations != nullptr)) == (a.cov3D_precomp != nullptr) || ((a.scales != nullptr) != (a.rotations != nullptr)))
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_forward: exactly one of (scales, rotations) / cov3D_precomp must be given");
    if (a.shs_rest && (!a.shs || a.M < 2)) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_forward: shs_rest needs shs (= features_dc) and M >= 2");
    if (a.raw_params && a.cov3D_precomp) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_forward: raw_params needs scales/rotations, not cov3D_precomp");
    if (a.shs && (a.D < 0 || a.D > 3)) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_forward: SH degree %d not in 0..3", a.D);
    if (a.shs && a.M < (a.D + 1) * (a.D + 1)) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_forward: M=%d < (D+1)^2=%d", a.M, (a.D + 1) * (a.D + 1));
    if (a.shs && !a.campos) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_forward: campos required with shs");
    return GSR_OK;
}
static int32_t fwd_preprocess(Call &c, PreprocessArgs &pa) {
    pa.gridx = c.pl.gridx; pa.gridy = c.pl.gridy; pa.exact_cull = c.o.exact_cull; pa.g = c.g; pa.seg_hdr = c.im.seg.hdr;
    pa.touch_mark = c.touch_mark = 1u + c.ds.frame_seq.fetch_add(1u) % 255u;
    HIP_TRY(launch_preprocess_fwd(pa, c.s), "preprocess launch");
    return c.debug ? hip_rc(hipStreamSynchronize(c.s), "preprocess") : GSR_OK;
}
static void fwd_totals(Call &c, uint32_t n32, uint32_t e32) { c.N = (int64_t)n32; c.E = (int64_t)e32; if (c.num_rendered) *c.num_rendered = c.N; }
static int32_t fwd_alloc_lists(Call &c, size_t extra, char **behind) {      // point_list + contrib, and `extra` bytes behind them (*behind)
    const size_t pl_bytes = carve_binning(nullptr, c.N, 0).list_bytes;
    char *ptr = (char *)c.alloc(c.alloc_user, pl_bytes + extra);
    if (!ptr) return fail(GSR_ERR_ALLOC, "binning allocator returned NULL for %zu bytes (N=%lld)", pl_bytes + extra, (long long)c.N);
    c.b = carve_binning(ptr, c.N, 0);
    if (behind) *behind = ptr + pl_bytes;
    return GSR_OK;
}
// default: entries binned per super-tile, every bin ordered in LDS (supertile_sort.hip).  lists_done stays false where that is not
// applicable, or a bin exceeds the LDS capacity / the entries the workspace: the frame then takes round 1's path (depth order + tile lists)
static int32_t fwd_lists_supertile(Call &c, const float *shs) {
    const SuperSortPlan ssp = super_sort_plan(c.P, c.W, c.H);
    if (c.o.tile_lists != 2 || !c.o.two_level_sort || c.debug || ssp.S > GSR_SS_MAXS || ssp.chunk > GSR_SS_MAX_CHUNK ||
        (size_t)ssp.S * ssp.nblk > (size_t)GSR_SS_WGCNT_WORDS) return GSR_OK;
    uint32_t h[4] = {1u, 0u, 0u, 0u};
    GSR_TRY(read_totals(c, "super-tile lists", [&](uint32_t *host_out, uint32_t seq) {
        hipError_t e = launch_super_sort_count(c.g, c.P, c.W, c.H, c.o.exact_cull, host_out, seq, c.s);
        if (e == hipSuccess) e = launch_super_sort_scatter(c.g, c.P, c.W, c.H, c.o.exact_cull, c.s);     // runs while the host waits for the totals
        return e;
    }, c.g.dord.hdr + SS_HDR_MAXBIN, h));
    if (h[0]) {      // round 1's path shares the (now dirty) counter region
        HIP_TRY(hipMemsetAsync(c.g.dord.hdr, 0, GSR_DO_ZERO_WORDS * sizeof(uint32_t), c.s), "reset counters");
        c.tm.mark(1); return GSR_OK;
    }
    fwd_totals(c, h[2], h[3]);
    GSR_TRY(fwd_alloc_lists(c, 0, nullptr));
    c.tm.zero(3); c.tm.zero(5); c.tm.mark(4);
    if (c.o.prefill_at == 2) GSR_TRY(prefill_fork(c.ds, c.s, shs, &c.pre));
    HIP_TRY(launch_super_sort_expand(c.g, c.im, c.b.point_list, c.P, c.W, c.H, h[1], c.s), "super-tile lists: order + expand");
    c.tm.mark(7);
    c.lists_done = true;
    return GSR_OK;
}
static int32_t fwd_depth_order_bucketed(Call &c, bool *ok) {      // depth_order.hip; !*ok: a bucket exceeds the LDS capacity -- general sort for this frame, log map next time
    uint32_t h[4] = {1u, 0u, 0u, 0u};
    const int log_map = c.ds.depth_log_map.load();
    GSR_TRY(read_totals(c, "depth order", [&](uint32_t *host_out, uint32_t seq) {
        hipError_t e = launch_depth_order_count(c.g, c.P, log_map, host_out, seq, c.s);
        if (e == hipSuccess) e = launch_depth_order_place(c.g, c.P, log_map, c.tile_lists ? 0 : 1, c.s);   // runs while the host waits for the totals
        if (e == hipSuccess && c.tile_lists) e = launch_tile_lists_count(c.g, c.P, c.g.dord.hdr, c.W, c.H, c.s);
        return e;
    }, nullptr, h));
    *ok = !h[0];
    if (*ok) { c.P_list = (int)h[1]; fwd_totals(c, h[2], h[3]); return GSR_OK; }
    int cur = c.ds.bucket_fail_p.load();          // under the robust map already: stop paying for the attempt at this size
    while (log_map && c.P < cur && !c.ds.bucket_fail_p.compare_exchange_weak(cur, c.P)) {}
    c.ds.depth_log_map.store(1);
    return GSR_OK;
}
static int32_t fwd_depth_order_general(Call &c) {      // rocPRIM's sort + scan; the totals come back by copy
    uint32_t n32 = 0, e32 = 0;
    HIP_TRY(launch_depth_sort(c.g, c.P, c.s), "depth sort");
    HIP_TRY(launch_ordered_scan(c.g, c.P, c.s), "ordered scan");
    HIP_TRY(launch_entry_total(c.g, c.P, c.s), "entry total");
    if (c.tile_lists) HIP_TRY(launch_tile_lists_count(c.g, c.P, nullptr, c.W, c.H, c.s), "tile lists: count");
    if (c.debug) HIP_TRY(hipStreamSynchronize(c.s), "depth order + scan");
    c.tm.mark(2);
    HIP_TRY(hipMemcpyAsync(&n32, c.g.offsets + (c.P - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c.s), "read N");
    HIP_TRY(hipMemcpyAsync(&e32, c.g.dord.hdr + DO_ETOT, sizeof(uint32_t), hipMemcpyDeviceToHost, c.s), "read E");
    HIP_TRY(hipStreamSynchronize(c.s), "read N sync");
    c.P_list = c.P; fwd_totals(c, n32, e32);
    return GSR_OK;
}
// yields P_list, N and E.  Whether tile_lists.hip will build the per-tile lists is known up front (image size, options): its level-1
// counting is queued before the host waits for N, and the depth order then skips the scan only key emission needs
static int32_t fwd_depth_order(Call &c) {
    c.tile_lists = c.o.tile_lists != 0 && c.o.two_level_sort && tile_list_plan(c.P, 0, c.W, c.H).S <= GSR_TL_MAX_S;
    bool bucketed = c.o.depth_buckets == 2 || (c.o.depth_buckets == 1 && c.P >= GSR_DEPTH_BUCKETS_MIN_P && c.P < c.ds.bucket_fail_p.load());
    if (bucketed) GSR_TRY(fwd_depth_order_bucketed(c, &bucketed));
    return bucketed ? GSR_OK : fwd_depth_order_general(c);
}
static int32_t fwd_lists_tile(Call &c) {      // per-tile lists from the depth order through (Gaussian, super-tile) entries (tile_lists.hip)
    const TileListPlan tlp = tile_list_plan(c.P, c.E, c.W, c.H);
    char *behind = nullptr;      // point_list first (what backward and the debug reader expect), then the entry workspace
    GSR_TRY(fwd_alloc_lists(c, carve_tile_lists(nullptr, tlp, c.E).total_bytes, &behind));
    const TileListView tv = carve_tile_lists(behind, tlp, c.E);
    c.tm.zero(3); c.tm.zero(5); c.tm.mark(4);           // no key emission / range detection on this path
    HIP_TRY(launch_tile_lists(c.g, tv, c.im, c.b.point_list, c.P, c.P_list, c.E, c.W, c.H, c.o.exact_cull, c.s), "tile lists");
    if (c.debug) HIP_TRY(hipStreamSynchronize(c.s), "tile lists");
    c.tm.mark(7);
    return GSR_OK;
}
static int32_t fwd_lists_sorted(Call &c) {      // key emission + rocPRIM sort + range detection
    size_t sort_tb = 0;
    const int tbits = tile_bits(c.W, c.H) > 0 ? tile_bits(c.W, c.H) : 1;
    HIP_TRY(any_sort_temp_bytes(c.N, c.W, c.H, &sort_tb), "sort temp query");
    c.b = carve_binning(nullptr, c.N, sort_tb);
    void *bin_ptr = c.alloc(c.alloc_user, c.b.total_bytes);
    if (!bin_ptr) return fail(GSR_ERR_ALLOC, "binning allocator returned NULL for %zu bytes (N=%lld)", c.b.total_bytes, (long long)c.N);
    c.b = carve_binning(bin_ptr, c.N, sort_tb);
    c.tm.mark(3);
    if (c.N > 0) {
        HIP_TRY(launch_emit_keys(c.g, c.b, c.P_list, c.W, c.H, c.o.exact_cull, c.o.two_level_sort, c.s), "emit keys launch");
        if (c.debug) HIP_TRY(hipStreamSynchronize(c.s), "emit keys");
        c.tm.mark(4);
        if (c.o.two_level_sort) HIP_TRY(launch_sort2_by_tile(c.b, c.N, tbits, c.s), "radix sort by tile");
        else HIP_TRY(launch_sort(c.b, c.N, key_bits(c.W, c.H), c.s), "radix sort");
        if (c.debug) HIP_TRY(hipStreamSynchronize(c.s), "radix sort");
    }
    c.tm.mark(5);
    HIP_TRY(launch_ranges(c.b, c.im, c.N, c.pl.T, c.o.two_level_sort, c.s), "tile ranges");
    if (c.debug) HIP_TRY(hipStreamSynchronize(c.s), "tile ranges");
    c.tm.mark(7);
    return GSR_OK;
}
static int32_t fwd_composite(Call &c, const float *bg, float *out_color) {
    CompositeArgs ca;
    ca.W = c.W; ca.H = c.H; ca.gridx = c.pl.gridx; ca.gridy = c.pl.gridy; ca.ranges = c.im.ranges; ca.point_list = c.b.point_list;
    ca.contrib = c.b.contrib; ca.contrib_stride = (size_t)(c.N > 0 ? c.N : 1);
    ca.rec = c.g.rec; ca.bg = bg; ca.final_T = c.im.final_T; ca.n_contrib = c.im.n_contrib; ca.out_color = out_color; ca.touched = c.g.touched; ca.touch_mark = c.touch_mark;
    ca.counters = lane_counters(c.ds, c.o.count_lanes, 0); ca.count_mode = c.o.count_lanes;
    // checkpoints + per-half-tile lengths for the segmented or the length-ordered reverse pass: only where gsr_backward will use them (Plan)
    ca.seg = c.im.seg; ca.seg_len = c.pl.seg_len; ca.asm_walk = c.o.asm_walk; ca.pair_long_n = c.pl.pair_long_n;
    ca.lpt_span = c.pl.seg_len == 0 && c.pl.T <= (1 << 28) ? c.pl.lpt_span : 0;
    HIP_TRY(launch_composite_fwd(ca, c.o.fwd_npx, c.o.exact_cull, c.o.wpb, c.s), "composite launch");
    return c.debug ? hip_rc(hipStreamSynchronize(c.s), "composite") : GSR_OK;
}

// ---- gsr_backward's stages, and its half of the decisions: what it adds to the shared Plan from R, the backward workspace, the lane counters and the pointers ----
struct Reverse {
    PergaussBwdArgs pa;            // inputs and gradient outputs as the per-Gaussian stage takes them: the checks and every stage read them here
    int64_t R;                     // pairs the forward pass rendered
    void *ws; size_t ws_bytes;     // the backward workspace as the caller gave it
    BackwardView w;                // and carved for this call's mode (bwd_workspaces)
    BinningView b; CompositeCounters *counters;   // the forward pass's lists; the instrumented reverse kernel's counters, or NULL
    bool det, persistent, lpt, dense, prefilled;
    int bwd_asm, pk_grid, fill_chunk;
};
static int32_t bwd_check(const Reverse &r, const float *bg, const float *dL_dpix, const void *geom_ws, const void *img_ws, const void *binning_ws) {
    const PergaussBwdArgs &a = r.pa;
    if (a.P < 0 || a.W <= 0 || a.H <= 0 || r.R < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward: bad sizes");
    if (a.P == 0) return GSR_OK;      // gsr_backward then has nothing to do
    if (!bg || !a.means3D || !a.radii || !a.viewmatrix || !a.projmatrix || !dL_dpix || !geom_ws || !img_ws || !r.ws ||
        !a.dL_dmeans2D || !a.dL_dopacity || !a.dL_dmeans3D)
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward: missing input, workspace or gradient buffer");
    if ((a.colors_precomp && !a.dL_dcolors) || (a.cov3D_precomp && !a.dL_dcov3D)) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward: dL_dcolors / dL_dcov3D required with colors_precomp / cov3D_precomp");
    if ((a.shs != nullptr) == (a.colors_precomp != nullptr)) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward: exactly one of shs / colors_precomp must be given");
    if (((a.scales != nullptr) && (a.rotations != nullptr)) == (a.cov3D_precomp != nullptr) || ((a.scales != nullptr) != (a.rotations != nullptr)))
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward: exactly one of (scales, rotations) / cov3D_precomp must be given");
    if (a.shs && (!a.dL_dsh || !a.campos || a.D < 0 || a.D > 3 || a.M < (a.D + 1) * (a.D + 1))) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward: SH inputs inconsistent");
    if (a.scales && (!a.dL_dscales || !a.dL_drots)) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward: dL_dscales/dL_drots required");
    if (a.shs_rest && (!a.shs || !a.dL_dsh_rest || a.M < 2)) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward: shs_rest needs shs, dL_dsh_rest and M >= 2");
    if (a.raw_params && a.cov3D_precomp) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward: raw_params needs scales/rotations");
    if (r.R > 0 && !binning_ws) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward: binning workspace missing");
    return GSR_OK;
}
static size_t det_slot_bytes(const Options &o, int64_t R) { return (size_t)R * (size_t)(4 / o.bwd_npx) * GSR_ACC_FLOATS * sizeof(float); }      // deterministic mode: one row per (list entry, wave of the tile)
static int32_t bwd_workspaces(const Call &c, Reverse &r, const void *binning_ws, size_t binning_bytes) {
    GSR_TRY(view_lists(binning_ws, binning_bytes, r.R, &r.b));
    if (acc_rows(c.P) >= (1u << 28)) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward: P too large for the 28-bit accumulator row index");
    r.det = c.o.deterministic_bwd != 0 && r.R > 0;
    r.w = carve_backward(r.ws, c.P, r.det ? det_slot_bytes(c.o, r.R) : 0);
    if (r.ws_bytes < r.w.acc_bytes) return fail(GSR_ERR_WORKSPACE, "backward workspace %zu < %zu", r.ws_bytes, r.w.acc_bytes);
    if (r.det && r.ws_bytes < r.w.det_end)
        return fail(GSR_ERR_WORKSPACE, "deterministic_bwd: backward workspace %zu < %zu (size it with gsr_backward_workspace_bytes)", r.ws_bytes, r.w.det_end);
    return GSR_OK;
}
static void bwd_plan(Call &c, Reverse &r) {      // which of the three reverse compositing kernels runs, and with what; the per-Gaussian stage's view of the workspaces
    r.counters = lane_counters(c.ds, c.o.count_lanes, 1);
    r.persistent = c.pl.persistent_bwd && r.R > 0;
    // the written-out reverse walk addresses the accumulator rows with a 32-bit byte offset: rows < 2^26
    r.bwd_asm = c.o.asm_walk && !r.det && (!r.counters || c.o.count_lanes == 2) && acc_rows(c.P) < (1u << 26) ? 1 : 0;
    // large images: half tiles in order of decreasing length (the forward pass filed the lengths when it ran with the same options)
    r.lpt = c.pl.lpt_span && !r.persistent && r.bwd_asm && !r.counters && r.R > 0 && c.o.wpb == 1;
    r.fill_chunk = r.persistent && c.o.fill_in_tail ? seg_fill_chunk(c.P) : 0;       // zero-fill units in the persistent kernel's lists
    r.pk_grid = r.persistent ? composite_bwd_persistent_grid(c.pl.T, r.det ? 1 : 0, count_variant(r.counters, c.o.count_lanes), r.bwd_asm, r.fill_chunk) : 0;
    r.pa.rec = c.g.rec; r.pa.clamped = c.g.clamped; r.pa.opac = c.g.opac; r.pa.hot = c.g.hot; r.pa.touched = c.g.touched; r.pa.touch_mark = c.g.touch_mark;
    r.pa.skip_unmarked = r.fill_chunk > 0 && r.R > 0 ? 1 : 0; r.pa.dense = 0;
    r.pa.vis_count = nullptr; r.pa.vis_list = nullptr; r.pa.vis_rec = nullptr; r.pa.vis_cap = 0;
}
// Dense per-Gaussian stage: the zeros of every gradient output are written by a kernel of their own on the device's second stream,
// forked by bwd_fork and joined in front of pergauss_bwd: it runs beside the compositing kernel (FP32-issue-bound, the memory system idle).
static void bwd_dense_setup(Call &c, Reverse &r) {
    r.dense = r.R > 0 && r.fill_chunk == 0 && c.pl.dense_wanted && pergauss_dense_eligible(r.pa) &&
              r.ws_bytes >= r.w.total_bytes;            // (a workspace sized before this stage existed: the streaming kernel)
    if (!r.dense) return;
    r.pa.vis_count = r.w.vis_count; r.pa.vis_list = r.w.vis_list; r.pa.vis_rec = r.w.vis_rec; r.pa.vis_cap = r.w.vis_cap;
    std::lock_guard<std::mutex> lk(c.ds.mu);
    if (!side_stream(c.ds)) r.dense = false;
}
// outputs the matching forward pass has zero-filled already (gsr_backward_prefill): no fill here, and the second stream's order
// (that fill, then this call's gathering kernel, then the join event) covers it.  Any other outstanding fill is joined first.
static int32_t bwd_take_prefill(Call &c, Reverse &r) {
    const PergaussBwdArgs &a = r.pa;
    r.prefilled = false;
    std::lock_guard<std::mutex> lk(c.ds.mu);
    if (!c.ds.prefill.done) return GSR_OK;
    c.ds.prefill.done = false;
    float *const outs[9] = {a.dL_dmeans2D, a.dL_dopacity, a.dL_dcolors, a.dL_dmeans3D, a.dL_dcov3D, a.dL_dsh, a.dL_dsh_rest, a.dL_dscales, a.dL_drots};
    r.prefilled = r.dense && c.ds.prefill.P == c.P && c.ds.prefill.M == a.M && !memcmp(outs, c.ds.prefill.p, sizeof outs);
    return r.prefilled ? GSR_OK : hip_rc(hipStreamWaitEvent(c.s, c.ds.ev_prefill, 0), "prefill join");
}
static int32_t bwd_fork(Call &c, const Reverse &r) {      // the second stream's work: gathering the Gaussians with a gradient, and the zeros unless the forward pass wrote them
    std::lock_guard<std::mutex> lk(c.ds.mu);
    HIP_TRY(hipEventRecord(c.ds.ev_fork, c.s), "fork event");
    HIP_TRY(hipStreamWaitEvent(c.ds.side, c.ds.ev_fork, 0), "fork wait");
    HIP_TRY(hipMemsetAsync(r.pa.vis_count, 0, 256, c.ds.side), "visible counter");
    HIP_TRY(launch_gather_visible(r.pa, c.ds.side), "gather launch");
    if (!r.prefilled) HIP_TRY(launch_fill_zero(r.pa, c.ds.side), "gradient zero-fill launch");
    return hip_rc(hipEventRecord(c.ds.ev_join, c.ds.side), "join event");
}
// Clears the accumulator rows (and builds the unit lists of the persistent or the length-ordered kernel), with the fork before or after:
// after, the clearing kernel has the chip to itself (7 us; 18 with the gathering kernel starting beside it) and the second stream's work
// starts with the compositing kernel -- config 3: 4 us better; at 5 M Gaussians the second stream's work (1.2 GB of zeros, 450 k records)
// outlasts the compositing kernel's shadow and every microsecond of head start counts: fork first (config 5: 2.37 against 2.42 ms)
static int32_t bwd_fork_and_clear(Call &c, const Reverse &r) {
    const int fork_late = c.o.dense_fork == 2 ? (c.P < GSR_DENSE_FORK_EARLY_P ? 1 : 0) : c.o.dense_fork;
    if (r.dense && !fork_late) GSR_TRY(bwd_fork(c, r));
    if (r.det) {
        HIP_TRY(hipMemsetAsync(r.ws, 0, r.w.det_end, c.s), "zero accumulators");
        if (r.persistent) HIP_TRY(launch_zero_marked_rows(c.P, c.g.touched, c.g.touch_mark, r.w.acc, 0, c.im.seg, r.pk_grid, r.fill_chunk, c.s), "unit lists");
    } else HIP_TRY(launch_zero_marked_rows(c.P, c.g.touched, c.g.touch_mark, r.w.acc, acc_rows(c.P), c.im.seg, r.persistent ? r.pk_grid : (r.lpt ? 1 : 0), r.fill_chunk, c.s), "zero accumulators");
    return r.dense && fork_late ? bwd_fork(c, r) : GSR_OK;
}
static int32_t bwd_composite(Call &c, const Reverse &r, const float *bg, const float *dL_dpix) {
    if (r.R <= 0) return GSR_OK;
    const PergaussBwdArgs &a = r.pa;
    CompositeBwdArgs ca;
    ca.W = c.W; ca.H = c.H; ca.gridx = c.pl.gridx; ca.gridy = c.pl.gridy; ca.ranges = c.im.ranges; ca.point_list = r.b.point_list;
    ca.contrib = r.b.contrib; ca.contrib_stride = (size_t)r.R;
    ca.rec = c.g.rec; ca.bg = bg; ca.final_T = c.im.final_T; ca.n_contrib = c.im.n_contrib; ca.dL_dpix = dL_dpix;
    ca.acc = r.w.acc; ca.det = r.w.det; ca.counters = r.counters; ca.count_mode = c.o.count_lanes;
    ca.P = c.P; ca.rect = c.g.rect; ca.tiles = c.g.tiles; ca.depth_bits = reinterpret_cast<const uint32_t *>(c.g.depth);
    ca.seg = c.im.seg; ca.asm_walk = r.bwd_asm;
    ca.fill.P = c.P; ca.fill.M = a.M; ca.fill.chunk = r.fill_chunk; ca.fill.radii = a.radii; ca.fill.touched = c.g.touched; ca.fill.mark = c.g.touch_mark;
    ca.fill.means2D = a.dL_dmeans2D; ca.fill.opacity = a.dL_dopacity; ca.fill.colors = a.dL_dcolors; ca.fill.means3D = a.dL_dmeans3D;
    ca.fill.cov3D = a.dL_dcov3D; ca.fill.sh = a.shs ? a.dL_dsh : nullptr; ca.fill.sh_rest = a.shs_rest ? a.dL_dsh_rest : nullptr;
    ca.fill.scales = a.scales ? a.dL_dscales : nullptr; ca.fill.rots = a.scales ? a.dL_drots : nullptr;
    if (r.persistent) HIP_TRY(launch_composite_bwd_persistent(ca, r.pk_grid, c.s), "composite backward launch");
    else if (r.lpt) HIP_TRY(launch_composite_bwd_lpt(ca, c.s), "composite backward launch");
    else HIP_TRY(launch_composite_bwd(ca, c.o.bwd_npx, c.o.wpb, c.s), "composite backward launch");
    return c.debug ? hip_rc(hipStreamSynchronize(c.s), "composite backward") : GSR_OK;
}
static int32_t bwd_pergauss(Call &c, Reverse &r) {      // joins the second stream in front of the per-Gaussian stage
    if (r.dense) {
        std::lock_guard<std::mutex> lk(c.ds.mu);
        HIP_TRY(hipStreamWaitEvent(c.s, c.ds.ev_join, 0), "join wait");
        r.pa.skip_unmarked = 1; r.pa.dense = 1;
    }
    HIP_TRY(launch_pergauss_bwd(r.pa, c.s), "per-Gaussian backward launch");
    return c.debug ? hip_rc(hipStreamSynchronize(c.s), "per-Gaussian backward") : GSR_OK;
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int32_t gsr_abi_version(void) { return GSR_ABI_VERSION; }
const char *gsr_last_error(void) { return g_err; }

// ---- options: one row per regular knob, walked by gsr_set_option and gsr_get_option alike; the irregular ones (per device, remapped,
// clamped, set-only, read-only) are explicit cases in the two functions.  include/gsr.h documents every name. ----
enum OptRule { OPT_BOOL, OPT_RANGE, OPT_1_2_4, OPT_MULT_64 };     // any value -> 0 / 1; lo..hi; 1, 2 or 4; 0 or a multiple of 64 up to hi
struct OptRow { const char *name; std::atomic<int> *var; OptRule rule; int lo, hi; const char *must; };
static const OptRow k_options[] = {
    {"exact_tile_cull", &g_exact_cull, OPT_BOOL, 0, 1, nullptr},
    {"two_level_sort", &g_two_level_sort, OPT_BOOL, 0, 1, nullptr},
    {"deterministic_bwd", &g_deterministic_bwd, OPT_BOOL, 0, 1, nullptr},
    {"fill_in_tail", &g_fill_in_tail, OPT_BOOL, 0, 1, nullptr},
    {"asm_walk", &g_asm_walk, OPT_BOOL, 0, 1, nullptr},
    {"bwd_lpt", &g_bwd_lpt, OPT_BOOL, 0, 1, nullptr},
    {"tile_lists", &g_tile_lists, OPT_RANGE, 0, 2, "0, 1 or 2"},
    {"persistent_bwd", &g_persistent_bwd, OPT_RANGE, 0, 2, "0, 1 or 2"},
    {"prefill_at", &g_prefill_at, OPT_RANGE, 0, 2, "0, 1 or 2"},
    {"dense_fork", &g_dense_fork, OPT_RANGE, 0, 2, "0, 1 or 2"},
    {"dense_pergauss", &g_dense_pergauss, OPT_RANGE, 0, 2, "0, 1 or 2"},
    {"depth_buckets", &g_depth_buckets, OPT_RANGE, 0, 2, "0, 1 or 2"},
    {"composite_waves_per_block", &g_wpb, OPT_1_2_4, 1, 4, "1, 2 or 4"},
    {"fwd_blocks_per_wave", &g_fwd_npx, OPT_1_2_4, 1, 4, "1, 2 or 4"},
    {"bwd_blocks_per_wave", &g_bwd_npx, OPT_1_2_4, 1, 4, "1, 2 or 4"},
    {"segment_entries", &g_seg_len, OPT_MULT_64, 0, 65536, "0 or a multiple of 64 up to 65536"},
};
static const OptRow *find_option(const char *name) {
    for (const OptRow &o : k_options) if (name && !strcmp(name, o.name)) return &o;
    return nullptr;
}
static bool option_accepts(const OptRow &o, int v) {
    if (o.rule == OPT_BOOL) return true;
    if (v < o.lo || v > o.hi) return false;
    return o.rule == OPT_1_2_4 ? v != 3 : o.rule == OPT_MULT_64 ? !(v & 63) : true;
}

int32_t gsr_set_option(const char *name, int32_t value) {
    if (const OptRow *o = find_option(name)) {
        if (!option_accepts(*o, value)) return fail(GSR_ERR_INVALID_ARGUMENT, "%s must be %s", o->name, o->must);
        o->var->store(o->rule == OPT_BOOL ? (value ? 1 : 0) : value);
        return GSR_OK;
    }
    if (name && !strcmp(name, "depth_log_map")) { DeviceState &ds = dev_state(); ds.depth_log_map.store(value ? 1 : 0); ds.bucket_fail_p.store(0x7fffffff); return GSR_OK; }
    if (name && !strcmp(name, "count_lanes")) { g_count_lanes.store(value == 2 ? 2 : (value ? 1 : 0)); return GSR_OK; }
    if (name && !strcmp(name, "composite_lds_pad")) { g_composite_lds_pad = value < 0 ? 0 : value; return GSR_OK; }     // set-only
    if (name && !strcmp(name, "fwd_pair_long")) { g_fwd_pair_long.store(value < -1 ? -1 : value); return GSR_OK; }
    return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_set_option: unknown option '%s'", name ? name : "(null)");
}
int32_t gsr_get_option(const char *name, int32_t *value) {
    if (name && value) {
        if (const OptRow *o = find_option(name)) { *value = o->var->load(); return GSR_OK; }
        if (!strcmp(name, "depth_log_map")) { *value = dev_state().depth_log_map.load(); return GSR_OK; }
        if (!strcmp(name, "count_lanes")) { *value = g_count_lanes.load(); return GSR_OK; }
        if (!strcmp(name, "fwd_pair_long")) { *value = g_fwd_pair_long.load(); return GSR_OK; }
        if (!strcmp(name, "pergauss_path")) { *value = pergauss_last_path(); return GSR_OK; }                          // read-only
        if (!strcmp(name, "poll_timeouts")) { *value = dev_state().poll_timeouts.load(); return GSR_OK; }              // read-only
    }
    return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_get_option: unknown option '%s'", name ? name : "(null)");
}

int32_t gsr_set_profiling(int32_t enable) { g_profiling.store(enable ? 1 : 0); return GSR_OK; }
int32_t gsr_get_stage_times(const char **names, float *ms) {
    DeviceState &ds = dev_state();
    std::lock_guard<std::mutex> lk(ds.mu);
    for (int i = 0; i < GSR_NUM_STAGES; i++) {
        if (names) names[i] = k_stage_names[i];
        if (ms) ms[i] = ds.stage_ms[i];
    }
    return GSR_OK;
}

int32_t gsr_workspace_sizes(int32_t P, int32_t W, int32_t H, size_t *geom_bytes, size_t *img_bytes, size_t *bwd_bytes) {
    if (P < 0 || W <= 0 || H <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_workspace_sizes: P=%d W=%d H=%d", P, W, H);
    if (W > 65535 * GSR_TILE_HOST || H > 65535 * GSR_TILE_HOST) return fail(GSR_ERR_INVALID_ARGUMENT, "image too large");
    GeomView g;
    GSR_TRY(view_geom(nullptr, SIZE_MAX, P, &g));
    if (geom_bytes) *geom_bytes = g.total_bytes;
    if (img_bytes) *img_bytes = carve_image(nullptr, W, H).total_bytes;
    if (bwd_bytes) *bwd_bytes = carve_backward(nullptr, P, 0).vis_off;      // the rows, rounded up: neither slots nor vis block
    return GSR_OK;
}

int32_t gsr_backward_workspace_bytes(int32_t P, int64_t R, size_t *bytes) {
    if (P < 0 || R < 0 || !bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward_workspace_bytes: bad argument");
    const Options o{};
    // with the dense per-Gaussian stage's list and record buffer (pergauss_bwd.hip), behind the accumulators
    *bytes = carve_backward(nullptr, P, o.deterministic_bwd ? det_slot_bytes(o, R) : 0).total_bytes;
    return GSR_OK;
}

int32_t gsr_binning_bytes(int64_t N, int32_t W, int32_t H, size_t *bytes) {
    if (N < 0 || W <= 0 || H <= 0 || !bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_binning_bytes: bad argument");
    size_t stb = 0;
    HIP_TRY(any_sort_temp_bytes(N, W, H, &stb), "sort temp query");
    *bytes = carve_binning(nullptr, N, stb).total_bytes;
    return GSR_OK;
}

int32_t gsr_forward(gsr_stream_t stream, int32_t P, int32_t D, int32_t M, int32_t W, int32_t H, const float *bg,
                    const float *means3D, const float *shs, const float *colors_precomp, const float *opacities,
                    const float *scales, float scale_modifier, const float *rotations, const float *cov3D_precomp,
                    const float *viewmatrix, const float *projmatrix, const float *campos, float tanfovx,
                    float tanfovy, int32_t prefiltered, int32_t debug, float *out_color, int32_t *radii, void *geom_ws,
                    size_t geom_bytes, gsr_alloc_fn binning_alloc, void *binning_user, void *img_ws, size_t img_bytes,
                    int64_t *num_rendered, const float *shs_rest, int32_t raw_params) {
    (void)prefiltered;   // culled Gaussians are always skipped, as with prefiltered=False (the only value the reference passes)
    Call c(stream, P, W, H, debug);
    c.alloc = binning_alloc; c.alloc_user = binning_user; c.num_rendered = num_rendered;
    fwd_totals(c, 0u, 0u);
    PreprocessArgs pa;
    pa.P = P; pa.D = D; pa.M = M; pa.W = W; pa.H = H; pa.raw_params = raw_params ? 1 : 0; pa.shs_rest = shs_rest; pa.radii = radii;
    pa.means3D = means3D; pa.shs = shs; pa.colors_precomp = colors_precomp; pa.opacities = opacities; pa.scales = scales; pa.rotations = rotations;
    pa.cov3D_precomp = cov3D_precomp; pa.viewmatrix = viewmatrix; pa.projmatrix = projmatrix; pa.campos = campos;
    pa.scale_modifier = scale_modifier; pa.tanfovx = tanfovx; pa.tanfovy = tanfovy;
    // an announcement is consumed whatever becomes of this call, and filled only where gsr_backward will take the dense per-Gaussian stage
    const bool fill = c.o.prefill_at != 0 && P > 0 && !debug && c.pl.dense_wanted && shs && !shs_rest && M == 16 && scales && rotations;
    GSR_TRY(prefill_take(c.ds, c.s, fill, P, M, &c.pre));
    GSR_TRY(fwd_check(pa, bg, out_color, geom_ws, img_ws, binning_alloc));
    if (P == 0) return hip_rc(hipMemsetAsync(out_color, 0, 3 * (size_t)W * H * sizeof(float), c.s), "memset out_color");   // as upstream: a zero image, not the background
    GSR_TRY(view_geom(geom_ws, geom_bytes, P, &c.g)); GSR_TRY(view_image(img_ws, img_bytes, W, H, &c.im));
    c.tm.mark(0);                                    // (the stages set the marks that fall between their own launches: 2, 3, 4, 5, 7)
    GSR_TRY(fwd_preprocess(c, pa));
    c.tm.mark(1);
    GSR_TRY(fwd_lists_supertile(c, shs));
    if (!c.lists_done) {
        GSR_TRY(fwd_depth_order(c));
        GSR_TRY(c.tile_lists && c.N > 0 ? fwd_lists_tile(c) : fwd_lists_sorted(c));
    }
    GSR_TRY(prefill_fork(c.ds, c.s, shs, &c.pre));
    GSR_TRY(fwd_composite(c, bg, out_color));
    prefill_publish(c.ds, c.pre);
    c.tm.mark(-1); c.tm.finish(11);
    return GSR_OK;
}

int32_t gsr_backward_prefill(int32_t P, int32_t M, float *dL_dmeans2D, float *dL_dopacity, float *dL_dcolors, float *dL_dmeans3D,
                             float *dL_dcov3D, float *dL_dsh, float *dL_dscales, float *dL_drots, float *dL_dsh_rest) {
    DeviceState &ds = dev_state();
    std::lock_guard<std::mutex> lk(ds.mu);
    ds.prefill.pending = false;
    if (P <= 0) return GSR_OK;               // withdraws an announcement
    if (M < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_backward_prefill: M < 0");
    float *const outs[9] = {dL_dmeans2D, dL_dopacity, dL_dcolors, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dsh_rest, dL_dscales, dL_drots};
    ds.prefill.P = P; ds.prefill.M = M;
    memcpy(ds.prefill.p, outs, sizeof outs);
    ds.prefill.pending = true;
    return GSR_OK;
}

int32_t gsr_backward(gsr_stream_t stream, int32_t P, int32_t D, int32_t M, int64_t R, int32_t W, int32_t H,
                     const float *bg, const float *means3D, const int32_t *radii, const float *shs,
                     const float *colors_precomp, const float *scales, float scale_modifier, const float *rotations,
                     const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, const float *campos,
                     float tanfovx, float tanfovy, const float *dL_dpix, const void *geom_ws, size_t geom_bytes,
                     const void *binning_ws, size_t binning_bytes, const void *img_ws, size_t img_bytes, void *bwd_ws,
                     size_t bwd_bytes, float *dL_dmeans2D, float *dL_dopacity, float *dL_dcolors, float *dL_dmeans3D,
                     float *dL_dcov3D, float *dL_dsh, float *dL_dscales, float *dL_drots, int32_t debug,
                     const float *shs_rest, int32_t raw_params, float *dL_dsh_rest) {
    Reverse r; PergaussBwdArgs &pa = r.pa;
    r.R = R; r.ws = bwd_ws; r.ws_bytes = bwd_bytes; pa.acc = (const float *)bwd_ws;
    pa.raw_params = raw_params ? 1 : 0; pa.shs_rest = shs_rest; pa.dL_dsh_rest = dL_dsh_rest;
    pa.P = P; pa.D = D; pa.M = M; pa.W = W; pa.H = H; pa.means3D = means3D; pa.shs = shs; pa.colors_precomp = colors_precomp; pa.radii = radii;
    pa.scales = scales; pa.rotations = rotations; pa.cov3D_precomp = cov3D_precomp; pa.viewmatrix = viewmatrix; pa.projmatrix = projmatrix;
    pa.campos = campos; pa.scale_modifier = scale_modifier; pa.tanfovx = tanfovx; pa.tanfovy = tanfovy;
    pa.dL_dmeans2D = dL_dmeans2D; pa.dL_dopacity = dL_dopacity; pa.dL_dcolors = dL_dcolors; pa.dL_dmeans3D = dL_dmeans3D;
    pa.dL_dcov3D = dL_dcov3D; pa.dL_dsh = dL_dsh; pa.dL_dscales = dL_dscales; pa.dL_drots = dL_drots;
    GSR_TRY(bwd_check(r, bg, dL_dpix, geom_ws, img_ws, binning_ws));
    if (P == 0) return GSR_OK;
    Call c(stream, P, W, H, debug);
    GSR_TRY(view_geom(geom_ws, geom_bytes, P, &c.g)); GSR_TRY(view_image(img_ws, img_bytes, W, H, &c.im));
    GSR_TRY(bwd_workspaces(c, r, binning_ws, binning_bytes));
    bwd_plan(c, r);
    c.tm.mark(8);
    bwd_dense_setup(c, r);
    GSR_TRY(bwd_take_prefill(c, r));
    GSR_TRY(bwd_fork_and_clear(c, r));
    c.tm.mark(9);
    GSR_TRY(bwd_composite(c, r, bg, dL_dpix));
    c.tm.mark(10);
    GSR_TRY(bwd_pergauss(c, r));
    c.tm.mark(-1); c.tm.finish(12);
    return GSR_OK;
}

int32_t gsr_mark_visible(gsr_stream_t stream, int32_t P, const float *means3D, const float *viewmatrix,
                         const float *projmatrix, uint8_t *present) {
    (void)projmatrix;
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mark_visible: bad argument");
    return hip_rc(launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream), "mark_visible launch");
}

int32_t gsr_composited_mask(gsr_stream_t stream, int32_t P, const void *geom_ws, size_t geom_bytes, uint8_t *out) {
    if (P < 0 || (P > 0 && (!geom_ws || !out))) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_composited_mask: bad argument");
    if (P == 0) return GSR_OK;
    GeomView g;
    GSR_TRY(view_geom(geom_ws, geom_bytes, P, &g));
    return hip_rc(launch_composited_mask(P, g.touched, g.touch_mark, out, (hipStream_t)stream), "composited mask launch");
}

int32_t gsr_debug_read_geom(gsr_stream_t stream, int32_t P, const void *geom_ws, float *depth, float *xy,
                            float *conic_opacity, float *rgb, uint32_t *tiles_touched, uint8_t *clamped) {
    hipStream_t s = (hipStream_t)stream;
    if (P <= 0) return GSR_OK;
    GeomView g;
    GSR_TRY(view_geom(geom_ws, SIZE_MAX, P, &g));
    HIP_TRY(hipStreamSynchronize(s), "sync");
    float *rec = (float *)malloc((size_t)P * GSR_REC_FLOATS * sizeof(float));
    uint8_t *cl = (uint8_t *)malloc((size_t)P);
    if (!rec || !cl) { free(rec); free(cl); return fail(GSR_ERR_ALLOC, "host malloc"); }
    hipError_t e = hipMemcpy(rec, g.rec, (size_t)P * GSR_REC_FLOATS * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(cl, g.clamped, (size_t)P, hipMemcpyDeviceToHost);
    if (e == hipSuccess && tiles_touched) e = hipMemcpy(tiles_touched, g.tiles, (size_t)P * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && depth) e = hipMemcpy(depth, g.depth, (size_t)P * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { free(rec); free(cl); return fail(GSR_ERR_HIP, "debug copy: %s", hipGetErrorString(e)); }
    for (int i = 0; i < P; i++) {
        const float *r = rec + (size_t)i * GSR_REC_FLOATS;
        if (xy) { xy[2 * i] = r[0]; xy[2 * i + 1] = r[1]; }
        if (conic_opacity) { conic_opacity[4 * i] = r[2]; conic_opacity[4 * i + 1] = r[3]; conic_opacity[4 * i + 2] = r[4]; conic_opacity[4 * i + 3] = r[5]; }
        if (rgb) { rgb[3 * i] = r[6]; rgb[3 * i + 1] = r[7]; rgb[3 * i + 2] = r[8]; }
        if (clamped) { clamped[3 * i] = cl[i] & 1; clamped[3 * i + 1] = (cl[i] >> 1) & 1; clamped[3 * i + 2] = (cl[i] >> 2) & 1; }
    }
    free(rec); free(cl);
    return GSR_OK;
}

int32_t gsr_debug_read_binning(gsr_stream_t stream, int64_t N, int32_t W, int32_t H, const void *binning_ws,
                               const void *img_ws, uint64_t *keys_sorted, uint32_t *point_list, uint32_t *ranges) {
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipStreamSynchronize(s), "sync");
    if (N > 0 && binning_ws) {
        BinningView b; GSR_TRY(view_lists(binning_ws, SIZE_MAX, N, &b));
        // the 64-bit tile<<32|depth keys only exist in global-sort mode (the other layouts may not even span that region)
        if (keys_sorted) {
            if (g_two_level_sort.load() == 0) HIP_TRY(hipMemcpy(keys_sorted, b.keys_sorted, (size_t)N * 8, hipMemcpyDeviceToHost), "copy keys");
            else memset(keys_sorted, 0, (size_t)N * 8);
        }
        if (point_list) HIP_TRY(hipMemcpy(point_list, b.point_list, (size_t)N * 4, hipMemcpyDeviceToHost), "copy point list");
    }
    if (ranges && img_ws) {
        ImageView im; GSR_TRY(view_image(img_ws, SIZE_MAX, W, H, &im));
        const size_t T = (size_t)grid_dim(W) * grid_dim(H);
        HIP_TRY(hipMemcpy(ranges, im.ranges, T * sizeof(uint2), hipMemcpyDeviceToHost), "copy ranges");
        if (point_list && N > 0) {
            // canonical (tile-major) order: tile_lists.hip lays the per-tile slices out super-tile-major; the
            // slices themselves are what the parity tests compare.  Empty tiles read (0, 0) as upstream's do.
            uint32_t *tmp = (uint32_t *)malloc((size_t)N * sizeof(uint32_t));
            if (!tmp) return fail(GSR_ERR_ALLOC, "host malloc");
            size_t pos = 0;
            for (size_t t = 0; t < T; t++) {
                const uint32_t a = ranges[2 * t], e = ranges[2 * t + 1];
                if (e <= a || (size_t)e > (size_t)N || pos + (e - a) > (size_t)N) { ranges[2 * t] = 0; ranges[2 * t + 1] = 0; if (e > a) { free(tmp); return fail(GSR_ERR_INVALID_ARGUMENT, "tile %zu: bad range [%u, %u)", t, a, e); } continue; }
                memcpy(tmp + pos, point_list + a, (size_t)(e - a) * sizeof(uint32_t));
                ranges[2 * t] = (uint32_t)pos; ranges[2 * t + 1] = (uint32_t)(pos + (e - a));
                pos += e - a;
            }
            if (pos != (size_t)N) { free(tmp); return fail(GSR_ERR_INVALID_ARGUMENT, "tile ranges cover %zu of %lld pairs", pos, (long long)N); }
            memcpy(point_list, tmp, (size_t)N * sizeof(uint32_t));
            free(tmp);
        }
    }
    return GSR_OK;
}

int32_t gsr_debug_read_lane_counters(uint64_t *fwd, uint64_t *bwd) {
    DeviceState &ds = dev_state();
    HIP_TRY(hipDeviceSynchronize(), "sync");
    std::lock_guard<std::mutex> lk(ds.mu);
    static_assert(sizeof(CompositeCounters) == 16 * sizeof(uint64_t), "counter block is 16 words");
    if (!ds.counters) {
        if (fwd) memset(fwd, 0, sizeof(CompositeCounters));
        if (bwd) memset(bwd, 0, sizeof(CompositeCounters));
        return GSR_OK;
    }
    if (fwd) HIP_TRY(hipMemcpy(fwd, ds.counters, sizeof(CompositeCounters), hipMemcpyDeviceToHost), "copy counters");
    if (bwd) HIP_TRY(hipMemcpy(bwd, ds.counters + 1, sizeof(CompositeCounters), hipMemcpyDeviceToHost), "copy counters");
    if (fwd) { fwd[9] = 0; fwd[10] = 0; }      // device pointer / capacity of the trace: not counters
    if (bwd) { bwd[9] = 0; bwd[10] = 0; }
    for (int w = 0; w < 2; w++)                 // reset the nine counters, keep the trace pointers
        HIP_TRY(hipMemset(ds.counters + w, 0, 9 * sizeof(unsigned long long)), "reset counters");
    return GSR_OK;
}

int32_t gsr_debug_read_wave_trace(int32_t which, uint32_t *out, int64_t max_units) {
    DeviceState &ds = dev_state();
    HIP_TRY(hipDeviceSynchronize(), "sync");
    std::lock_guard<std::mutex> lk(ds.mu);
    if (which < 0 || which > 1 || !out || max_units < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_debug_read_wave_trace: bad argument");
    if (!ds.counters) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_debug_read_wave_trace: count_lanes has not run on this device");
    const size_t n = (size_t)(max_units < (int64_t)GSR_TRACE_UNITS ? max_units : (int64_t)GSR_TRACE_UNITS);
    const char *base = reinterpret_cast<const char *>(ds.counters + 2) + (size_t)which * GSR_TRACE_UNITS * sizeof(uint4);
    HIP_TRY(hipMemcpy(out, base, n * sizeof(uint4), hipMemcpyDeviceToHost), "copy trace");
    HIP_TRY(hipMemset(const_cast<char *>(base), 0, (size_t)GSR_TRACE_UNITS * sizeof(uint4)), "reset trace");
    return GSR_OK;
}

int32_t gsr_debug_read_bound_errors(gsr_stream_t stream, int32_t P, const void *geom_ws, int32_t W, int32_t H, const void *img_ws, uint32_t *out) {
    hipStream_t s = (hipStream_t)stream;
    if (!out) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_debug_read_bound_errors: bad argument");
    memset(out, 0, 12 * sizeof(uint32_t));
#ifdef GSR_DEBUG_BOUNDS
    out[8] = 1u;
#endif
    HIP_TRY(hipStreamSynchronize(s), "sync");
    if (geom_ws && P > 0) {
        GeomView g;
        GSR_TRY(view_geom(geom_ws, SIZE_MAX, P, &g));
        HIP_TRY(hipMemcpy(out, g.dord.hdr + GSR_DBG_GEOM_WORD, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost), "copy bound words");
    }
    if (img_ws && W > 0 && H > 0) {
        ImageView im; GSR_TRY(view_image(img_ws, SIZE_MAX, W, H, &im));
        HIP_TRY(hipMemcpy(out + 4, im.seg.hdr + GSR_DBG_SEG_WORD, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost), "copy bound words");
        // self test of the mechanism, on words of its own (seg.hdr[8..11])
        HIP_TRY(hipMemsetAsync(im.seg.hdr + 8, 0, 4 * sizeof(uint32_t), s), "clear self-test words");
        HIP_TRY(launch_bound_selftest(im.seg.hdr + 8, s), "bound self test");
        HIP_TRY(hipStreamSynchronize(s), "sync");
        uint32_t st[4];
        HIP_TRY(hipMemcpy(st, im.seg.hdr + 8, sizeof(st), hipMemcpyDeviceToHost), "copy self-test words");
        out[9] = st[0]; out[10] = st[1]; out[11] = st[2];
    }
    return GSR_OK;
}

int32_t gsr_debug_read_segments(gsr_stream_t stream, int32_t W, int32_t H, const void *img_ws, uint32_t *summary) {
    hipStream_t s = (hipStream_t)stream;
    if (!img_ws || !summary || W <= 0 || H <= 0) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_debug_read_segments: bad argument");
    HIP_TRY(hipStreamSynchronize(s), "sync");
    ImageView im; GSR_TRY(view_image(img_ws, SIZE_MAX, W, H, &im));
    uint32_t *h = (uint32_t *)malloc(GSR_SEG_HDR_WORDS * sizeof(uint32_t));
    if (!h) return fail(GSR_ERR_ALLOC, "host malloc");
    const hipError_t e = hipMemcpy(h, im.seg.hdr, GSR_SEG_HDR_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { free(h); return fail(GSR_ERR_HIP, "copy segment header: %s", hipGetErrorString(e)); }
    uint32_t units = 0, slots = 0, drawn = 0;
    for (int b = 0; b < GSR_SEG_BANDS; b++) {
        units += h[SEG_BCOUNT + b];
        const uint32_t share = im.seg.pool_cap / GSR_SEG_BANDS, got = h[SEG_POOL + GSR_SEG_CTR_STRIDE * b];
        slots += got < share ? got : share;
        drawn += h[SEG_BTICKET + GSR_SEG_CTR_STRIDE * b];
    }
    summary[0] = h[SEG_SEG]; summary[1] = units; summary[2] = slots; summary[3] = im.seg.pool_cap; summary[4] = im.seg.units; summary[5] = drawn;
    summary[6] = 0; summary[7] = 0;
    free(h);
    return GSR_OK;
}

int32_t gsr_debug_read_image_state(gsr_stream_t stream, int32_t W, int32_t H, const void *img_ws, float *final_T,
                                   uint32_t *n_contrib) {
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipStreamSynchronize(s), "sync");
    ImageView im; GSR_TRY(view_image(img_ws, SIZE_MAX, W, H, &im));
    const size_t HW = (size_t)W * H;
    if (final_T) HIP_TRY(hipMemcpy(final_T, im.final_T, HW * 4, hipMemcpyDeviceToHost), "copy final_T");
    if (n_contrib) HIP_TRY(hipMemcpy(n_contrib, im.n_contrib, HW * 4, hipMemcpyDeviceToHost), "copy n_contrib");
    return GSR_OK;
}

}  // extern "C"
