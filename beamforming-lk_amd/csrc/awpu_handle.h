// awpu_handle.h -- internal to libawpu_hip.so: the handle, the error helpers, and what its three host files call in one another:
// awpu_hip.cpp (the C ABI and its call paths), awpu_sweep.cpp (tables, launchers, dispatch) and awpu_runs.cpp (the runs of blocks).
// Nothing here is part of the C ABI.
#pragma once

#include "awpu_hip.h"
#include "awpu_hip_track.h"

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "das_kernels.h"

namespace awpu::host {

void note_error(const std::string &text);  // the calling thread's last error, and that of the handle it is working on

// the handle the calling thread is working on: errors are also kept in the handle, so that a thread
// other than the one that ran into the error (a GUI thread asking about a worker's engine) can read them
struct CtxScope {
    awpu_hip *saved;
    explicit CtxScope(awpu_hip *h);
    ~CtxScope();
};
#define AWPU_CTX(h) awpu::host::CtxScope ctx_scope_(h)

int hip_fail(hipError_t e, const char *what);

#define AWPU_HIP_TRY(call)                                           \
    do {                                                             \
        hipError_t e_ = (call);                                      \
        if (e_ != hipSuccess) return awpu::host::hip_fail(e_, #call); \
    } while (0)

int invalid(const char *why);
int fail(int status, const char *why);

template <class T>
void dev_free(T *&p) {  // hipFree + forget
    if (p) (void) hipFree(p);
    p = nullptr;
}

// Two buffers of `cap` bytes each for the two pieces a run has in flight (piece i uses [i & 1]): device memory, pinned host
// memory, or both.  Grow-only; a failed allocation leaves cap 0 and whatever was allocated, which the next ensure() frees.
struct BufferPair {
    unsigned char *d[2] = {nullptr, nullptr}, *h[2] = {nullptr, nullptr};
    size_t cap = 0;
    int ensure(size_t bytes, bool want_host, bool want_device = true);
    void release();
};

// The quad-major tables (awpu_sweep.cpp, build_quad_lut), one per layout: what the table's LDS addresses point into
enum QuadLayout {
    kQuadPairs = 0,           // the quad shape's frame pairs (das_quad_kernel)
    kQuadExactNd,             // {next, d} of a frame pair (das_exact_nd_kernel): 16-byte elements, quad rows padded to an even count
    kQuadHalves,              // the halves layout of single frames (das_quadh_kernel)
    kQuadHalvesStationary,    // ... with slot = mic (das_quadh_stationary_kernel: every mic's row resident)
    kQuadExact,               // raw sample pairs (das_exact_quad_kernel): the image, and the plan, of the exact pair table
    kQuadExactNdh,            // single frames: the halves form of {next, d}, chunked (das_exact_ndh_kernel, das_exact_ndp_kernel)
    kQuadExactNdhStationary,  // ... every mic resident
    kQuadLayouts
};
struct QuadTable {
    awpu::QuadEntry *d = nullptr;
    size_t entries = 0;  // allocated (the launchers check their kernel's reach against it: das_kernels.h, Extents)
    awpu::FastPlan plan{};  // set by prepare() where the window fits the layout's image
};

}  // namespace awpu::host

struct awpu_hip {
    awpu_hip_cfg cfg{};
    hipStream_t stream = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    bool timing = true;

    // host copies of what the reference keeps in MIMOWorker / Antenna
    std::vector<int32_t> off;   // [pixel_count][lut_stride]  offsetDelays
    std::vector<float> frac;    // [pixel_count][lut_stride]  fractionalDelays
    std::vector<int32_t> index; // [usable]                   antenna.index
    std::vector<float> gain;    // [n_streams] optional per-mic gain (awpu_hip_set_mic_gains); empty = none
    bool have_table = false, have_mics = false, prepared = false;

    // device state
    awpu::LutEntry *d_lut = nullptr;
    struct FastLut {
        awpu::FastPlan plan;
        awpu::FastEntry *d = nullptr;
        size_t entries = 0;  // allocated (the launchers check their kernel's reach against it: das_kernels.h, Extents)
    };
    std::vector<FastLut> fast_luts;  // one per (frames per item, LDS image size) in use
    awpu::FastEntry *d_exact_pair_lut = nullptr;  // reference-order sweep on the frame-pair layout (das_exact_pair_kernel)
    size_t exact_pair_lut_entries = 0, fir_plane_lut_entries = 0;  // allocated entries of the table above and of the FIR8 plane table
    awpu::FastPlan exact_plan{};                  // ... its plan, and that of quad_tables[kQuadExact]
    awpu::host::QuadTable quad_tables[awpu::host::kQuadLayouts];  // the quad-major tables, by QuadLayout
    unsigned *d_nd_queue = nullptr;               // das_exact_nd_kernel's eight item counters (one per XCD)
    int2 *d_nd_items = nullptr;                   // ... and its item list (nd_items_kernel), valid for nd_items_key
    size_t nd_items_cap = 0;
    long long nd_items_key = -1;                  // (n_pairs, pair group, quads per wave) the list was built for; -1: none
    int n_cus = 0;                                // compute units of the handle's device (persistent workgroups: one per CU)
    bool exact_nd_ok = false;     // ... and the window fits the {next, d} image (kQuadExactNd)
    // single frames: ... its halves form, chunked / every mic resident; fast_ndp_ok: AWPU_MATH_F32_FAST takes the chunked one on small grids
    bool exact_ndh_ok = false, exact_ndhs_ok = false, fast_ndp_ok = false;
    bool identity_mics = false;   // the active-mic list is 0 .. usable-1 (awpu_hip_set_active_mics(NULL)): rows need no look-up
    bool exact_pairs_ok = false;  // AWPU_MATH_F32_EXACT + LERP and the window fits the pair image
    float *sums_out = nullptr;    // awpu_hip_process_device_sums: where the launch in progress exports out[] (else null)
    void *d_fir_plane_lut = nullptr;           // FIR8 on the four-plane layout: one dword per (pixel, mic): address, plane, coefficient row
    awpu::FastPlan fir_plane_plan{};
    bool fir_planes_ok = false;                // AWPU_MATH_F32_FAST + FIR8 and the window fits the plane image
    std::vector<float> fir;                    // host copy of the [101][8] coefficient table (baked into the plane entries)
    bool quadh_fits = false;      // single frames on the halves layout (das_quadh_kernel)
    bool quadhs_fits = false;     // ... with every active mic's row in LDS at once (das_quadh_stationary_kernel: one 8x8 array does)
    bool quad_ok = false;         // the table's statistics favour the quad shape (decided in prepare)
    double quad_cost = 0.0;       // its expected packed VALU instructions per quad and mic (32 = no sharing at all)
    double quad_differ = 3.0;     // pixels of a vertical quad (of three) whose integer delay differs from the second pixel's, per mic (table sample)
    int32_t *d_index = nullptr;
    float *d_gain = nullptr;  // [usable] gains in active-mic order, or null
    float *d_calib = nullptr; // [64] per-mic mean squares (calibration)
    awpu::LutEntry *d_beam_lut = nullptr;  // [beam_cap][usable] entries of awpu_hip_beams
    float *d_beam_out = nullptr;           // [beam_cap] powers then [beam_cap][256] beams
    size_t beam_cap = 0, beam_lut_cap = 0;
    // particle tracking (awpu_hip_track.h)
    std::vector<float> antenna;            // [3][antenna_n] element positions by stream id (awpu_hip_set_antenna); empty = none
    float *d_xyz = nullptr;                // ... on the device
    std::vector<int32_t> track_index;      // the active mics d_track_index holds
    int32_t *d_track_index = nullptr;
    size_t track_index_cap = 0;
    unsigned char *d_track = nullptr;      // particles, then the reference used, then [n][256] beams (steer_table_device: angles, tables)
    size_t track_cap = 0;                  // bytes
    float *d_fir = nullptr;  // [101][8] coefficient table (AWPU_INTERP_FIR8)
    float *d_ring = nullptr;            // [n_streams][2048] history ring (awpu_hip_ingest_block)
    uint8_t *d_display = nullptr;       // awpu_hip_live_block: peak (one float), compact image, upscaled image
    size_t display_cap = 0;             // bytes
    awpu::ResizeTap *d_taps = nullptr;  // column + row taps of the display upscale, for taps_key
    int taps_key[4] = {0, 0, 0, 0};     // {srows, scols, drows, dcols}
    int taps_band_rows = 0;             // ... and the most compact rows a 16-row tile of the large image reads (watch_kernels.h)
    float *d_pack = nullptr;            // [pairs][usable][wp][2] sample-interleaved frame pairs
    size_t pack_cap = 0;                // floats
    unsigned char *d_datagrams = nullptr;  // staging for one block of wire datagrams
    int32_t *d_row_off_ring = nullptr;  // row offsets for frames read out of the ring (pitch 2048)
    int ring_pos = 0;                   // where the next block goes = start of the snapshot
    // awpu_hip_live_block as a HIP graph: the call's copies and launches captured once per (ring position, caller
    // buffers, table generation) and replayed with one hipGraphLaunch
    struct LiveGraph {
        int ring_pos, stride, rows, cols, out_rows, out_cols;
        const void *datagrams, *power, *image, *colormap, *big_image;
        unsigned long long gen;
        hipGraphExec_t exec;
        unsigned long long last_use;  // live_clock at the last replay: the least recently used graph is evicted
    };
    std::vector<LiveGraph> live_graphs;
    unsigned long long table_gen = 0;   // bumped whenever prepare() rebuilds the device tables
    int live_warm = 0;                  // plain live calls made with the current tables AND this call shape (lazy allocations done after one)
    unsigned long long live_shape = 0;  // the shape those calls had: image sizes, which outputs, colour table or not
    const void *live_bufs[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // ... and the caller's buffers (a capture bakes them in)
    unsigned long long live_clock = 0;
    bool live_graph_broken = false;     // a capture failed on this runtime: never try again
    bool have_fir = false;
    int32_t *d_row_off = nullptr;
    int32_t *d_row_off_compact = nullptr;  // the same for frames uploaded as [streams][compact_hist] windows
    int compact_hist = 0;                  // 0 = the window cannot be cut out (it touches the newest sample)
    float *d_frames = nullptr;
    float *h_live_in = nullptr, *h_live_out = nullptr;  // pinned staging of awpu_hip_process's one-frame calls (the live path): window in, powers out
    size_t live_in_cap = 0, live_out_cap = 0;           // in floats
    unsigned live_calls = 0;                            // ... how many of them this handle has served (every 32nd is timed by events)
    // ... their completion flag (the resident single-frame kernels with one quad per wave): the device counter the workgroups count themselves on, what it will read
    // when every launch armed so far is over, the pinned flag and the sequence number of the last armed launch
    unsigned long long *d_done_counter = nullptr, done_total = 0;
    unsigned *h_done_flag = nullptr, done_seq = 0;
    bool done_arm = false, done_used = false;           // arm: the next single-frame sweep is to raise the flag; used: it will
    float *d_power = nullptr;
    size_t frames_cap = 0, power_cap = 0;  // in floats
    int wstart = 0, window = 0, tau_max = 0;
    int pair_cols = 0;  // frame-pair sweep: > 0 = waves take vertically adjacent pixels (grid row length), 0 = consecutive

    // device group (cfg.n_devices > 1): this handle owns no sweep state of its own, only one part per device
    std::vector<awpu_hip *> parts;
    // a part's pixels inside the group's range: (first pixel relative to the group's pixel_begin, count), ascending; the part's
    // own table and power rows hold them back to back.  One range = a contiguous slab; several = row groups of four dealt
    // round-robin over the devices (edge rows of the sine-space grid cost the quad shapes more than centre rows: DESIGN.md 6)
    std::vector<std::pair<int, int>> ranges;
    bool union_window_done = false;  // group: every part stages the union of the parts' windows (packed frames need one layout)
    hipEvent_t ev_fan = nullptr;            // group: recorded on the caller's stream, awaited by every part
    // a part's share of the fan-out (awpu_hip_process_device on a group): two window buffers, so that the copy of
    // call k+1 (on copy_stream) runs beside the sweep of call k (on stream)
    hipStream_t copy_stream = nullptr;
    float *d_fan[2] = {nullptr, nullptr};
    size_t fan_cap = 0;                     // floats per buffer
    hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_swept[2] = {nullptr, nullptr}, ev_done = nullptr;
    unsigned fan_turn = 0;
    // how a part of a group reaches devices[0]: kPeerSame (the same GPU), kPeerDirect (peer copies over xGMI) or
    // kPeerStaged (no peer access on this node: the window and the tiles cross pinned host memory, explicitly)
    int peer = 0;
    float *h_stage[2] = {nullptr, nullptr};  // group: pinned staging of the frames' window for the staged parts
    size_t stage_cap = 0;                    // floats per buffer
    int stage_lo = 0, stage_w = 0;           // group: the window [stage_lo, stage_lo + stage_w) of every stream that is staged
    hipEvent_t ev_staged[2] = {nullptr, nullptr};   // group: window b is in h_stage[b]
    unsigned stage_turn = 0;
    float *h_tile[2] = {nullptr, nullptr};   // part (staged): pinned staging of its power tile on the way back
    size_t tile_cap = 0;
    hipEvent_t ev_tile_free[2] = {nullptr, nullptr};  // part (staged): the caller's stream has read h_tile[b]
    hipEvent_t ev_staged_read[2] = {nullptr, nullptr};  // part (staged): its upload out of the group's h_stage[b] is done
    bool stage_used[2] = {false, false};
    bool tile_used[2] = {false, false}, fan_used[2] = {false, false};
    bool in_flight = false;                 // awpu_hip_process_async without its awpu_hip_wait yet
    // runs of blocks (awpu_runs.cpp), by piece: piece i's history [n_streams][768 + 256 * piece] in blk_hist.d[i & 1], its windows
    // in d_blk_frames; the host forms stage piece i's input in pinned blk_in.h[i & 1], upload it to blk_in.d[i & 1] on copy_stream
    // and bring its powers back through pinned blk_out.h[i & 1]
    awpu::host::BufferPair blk_hist, blk_in, blk_out;
    float *d_blk_frames = nullptr;
    size_t blk_frames_cap = 0;  // floats
    // ev_blk_in[b]: blk_in.h[b] may be refilled; ev_blk_hist[b]: blk_hist.d[b] formed; ev_blk_cut[b]: ... and read by the cut;
    // ev_blk_swept[b]: d_power's half b holds its piece's powers; ev_blk_out[b]: ... and blk_out.h[b] too; ev_blk_ring: orders a
    // run after the work queued on the handle's stream, and the handle's stream after a device-form run on the caller's stream
    hipEvent_t ev_blk_in[2] = {nullptr, nullptr}, ev_blk_hist[2] = {nullptr, nullptr}, ev_blk_cut[2] = {nullptr, nullptr},
               ev_blk_swept[2] = {nullptr, nullptr}, ev_blk_out[2] = {nullptr, nullptr}, ev_blk_ring = nullptr;
    // listening to such runs (awpu_hip_listen.h): the listeners on the device from piece to piece; the host forms get piece i's
    // audio rows [n][256 * piece], then its trail, in listen_out.d[i & 1] and bring them back through pinned listen_out.h[i & 1].
    // listen_stream: where the listen kernels run beside the sweeps when heatmaps are asked for too.
    unsigned char *d_listeners = nullptr;
    size_t listeners_cap = 0;  // bytes
    awpu::host::BufferPair listen_out;
    hipStream_t listen_stream = nullptr;
    // ev_listened[b]: the listen kernels have read blk_hist.d[b] (and written listen_out.d[b]); ev_listen_out[b]: listen_out.h[b] holds it
    hipEvent_t ev_listened[2] = {nullptr, nullptr}, ev_listen_out[2] = {nullptr, nullptr};

    // watching such runs (awpu_hip_watch.h): piece i's peaks, compact images and (host forms) large images in watch.d[i & 1]; the
    // host forms bring the images back through pinned watch.h[i & 1].  The events are those of the runs above: ev_blk_swept[b] is
    // recorded behind the display kernels, ev_blk_out[b] behind the images' way back.
    awpu::host::BufferPair watch;

    awpu_hip_stats stats{};
    std::string last_error;                  // awpu_hip_last_error_of
    unsigned long long *d_diag = nullptr;    // AWPU_FAST_DEBUG=16 cycle stamps of the last launch
    size_t diag_cap = 0;                     // in 64-bit words

    int usable() const { return static_cast<int>(index.size()); }
};

namespace awpu::host {

// What the process environment can change.  The SHIPPING library reads three variables, none of them needed in production:
//   AWPU_SHAPE             force one of the production sweep shapes wherever it can serve the call (tests sweep every shape
//                          through the oracle this way; the default rule -- launch() -- picks by table statistics and launch size):
//                          pair | pair_vertical | pair_horizontal | quad | noquad | stationary | quadh | quadh_chunked | single_db | single_small |
//                          fir8_planes | exact_pair | exact_quad | exact_nd1 | exact_nd2 | exact_ndp | exact_verify
//   AWPU_LIVE_GRAPH=0      awpu_hip_live_block always enqueues its steps one by one (no HIP-graph replay)
//   AWPU_GROUP_FORCE_COPY  device groups: 1 = a part on devices[0] takes the window-copy path too, 2 = through pinned host
//                          memory (how one GPU exercises the paths a part on another GPU takes)
// Everything else -- chunk geometry, XCD pair groups, persistent workgroups, priority variants, cycle stamps -- exists only in
// builds with -DAWPU_TUNING_BUILD (AWPU_EXTRA_HIPCC_FLAGS; -DAWPU_TIMING_BUILD implies it), which read the round-1..3 variables
// (AWPU_FAST_*, AWPU_FIR8_*, AWPU_QUAD_VARIANT, AWPU_EXACT_PAIRS) as before.  Read once per process.
struct EnvKnobs {
    int fpi = 0, ppw = 0, nw = 0;  // single-frame shape forced: frames per item (always 1 here), pixels per wave, 8 / 32
    int pairs = -1;                // 0 / 1: never / always a frame-pair sweep (quad, stationary or pair shape) for batches >= 2
    int debug = 0;                 // AWPU_FAST_DEBUG bits (tuning builds)
    int fpw = 0;                   // tuning: consecutive frames per workgroup of the double-buffered single-frame shape
    int quads = -1;                // 0 / 1: never / always (where the row length is known) the quad shapes
    int pair_group = 0;            // tuning: frame pairs an XCD works on at a time (quad shape)
    int quad_variant = 0;          // tuning: block variant (AWPU_QUAD_VARIANT)
    int stationary = -1;           // 0 / 1: never / always (where the window fits the LDS) the stationary pair shape
    int fir_planes = 1;            // 2: the four-plane FIR8 kernel for every batch >= 2 however small the grid
    int fir_share = 1;             // tuning: 0 = the FIR8 plane kernel sweeps four consecutive pixels even where the row length is known
    int wgs = 0;                   // tuning: persistent workgroups of the quad shape (0 = default rule, -1 = one workgroup per item)
    int live_graph = 1;            // AWPU_LIVE_GRAPH
    int halves = -1;               // 1: single frames on the halves layout for every call (where the quad table is built)
    int exact_pairs = 1;           // 0: AWPU_MATH_F32_EXACT on the round-1 verification kernel (das_exact_kernel)
    int pair_cols = -1;            // 0 / 1: the pair shape pairs consecutive / vertically adjacent pixels (default: whichever coincides more)
    int group_copy = 0;            // AWPU_GROUP_FORCE_COPY
    int listen_stream = 1;         // tuning: 0 = the listen kernels queue behind the sweeps instead of running beside them
    EnvKnobs();
};
const EnvKnobs &env();

// layout of d_frames: kFull [batch][n_streams][hist]; kCompact [batch][n_streams][compact_hist] with
// sample 0 = history sample wstart; kRing one frame read in place from the ingest ring (rows 2048 apart)
enum FrameLayout { kFull = 0, kCompact = 1, kRing = 2 };

// the sweep layer: defined, and described, in awpu_sweep.cpp
int prepare(awpu_hip *h);
void free_tables(awpu_hip *h);
int launch(awpu_hip *h, const float *d_frames, int batch, float *d_power, hipStream_t s, int layout = kFull);
bool takes_packed_pairs(awpu_hip *h, int batch, awpu::FastPlan *plan);
int packed_shape(awpu_hip *h, int batch, awpu::FastPlan *plan);
size_t packed_floats_of(const awpu_hip *h, const awpu::FastPlan &plan, int batch);
int pack_for_sweep(awpu_hip *h, const awpu::FastPlan &plan, const float *d_frames, int batch, float *d_packed, hipStream_t s);
int sweep_packed(awpu_hip *h, const awpu::FastPlan &plan, const float *d_packed, size_t packed_floats, int batch, float *d_power, hipStream_t s);

// defined, and described, in awpu_hip.cpp
void retire_live_graphs(awpu_hip *h);
int check_ready(awpu_hip *h, int batch);
int ensure_power(awpu_hip *h, size_t need_power);
int ensure_ring(awpu_hip *h);
int host_piece(int batch);
int wait_and_time(awpu_hip *h);
size_t align16(size_t n);
int check_particles(const awpu_particle_t *p, int32_t n, double theta_limit, double reference);
int check_antenna(const awpu_hip *h);
int ensure_track_index(awpu_hip *h);
int ensure_taps(awpu_hip *h, int rows, int cols, int out_rows, int out_cols, hipStream_t s);

}  // namespace awpu::host
