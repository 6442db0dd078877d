// awpu_handle.h -- internal to libawpu_hip.so: the handle, the owner types of what it holds on the device, the error helpers, and
// what its host files call in one another: awpu_hip.cpp (the C ABI and its call paths), awpu_group.cpp (the device group),
// awpu_sweep.cpp (tables, launchers, dispatch), awpu_focus.cpp (candidate distances), and the runs of blocks: run_pieces.cpp (the
// pipeline; run_pieces.h), watch_run.cpp (the display step; watch_run.h), awpu_runs.cpp (blocks, listen, watch, find, locate) and one
// file per feature with all of its calls -- awpu_spectral.cpp, awpu_expose.cpp, awpu_cohere.cpp, awpu_peel.cpp.  Nothing here is
// part of the C ABI.
#pragma once

#include "awpu_hip.h"
#include "awpu_hip_spectral.h"
#include "awpu_hip_tones.h"
#include "awpu_hip_track.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
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

// ---- owner types: whatever the handle holds on the device frees itself with the handle.  A new buffer, event or stream needs its
// declaration and nothing else.  Non-copyable, usable wherever the raw pointer / event / stream is; only the buffers are movable.

struct DeviceMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void *p) { (void) hipFree(p); }
    static constexpr const char *what = "hipMalloc";
};
template <unsigned Flags>
struct PinnedMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
    static void free(void *p) { (void) hipHostFree(p); }
    static constexpr const char *what = "hipHostMalloc";
};

// A grow-only buffer of T: ensure(n) leaves it holding at least n elements.  Growing frees first (hipFree waits for the device:
// launches still reading the old buffer finish first), asks for exactly n, and a failed allocation leaves it empty -- cap 0 --
// for the next call to try again.  Contents do not survive growing.
template <class T, class Mem>
struct Buffer {
    T *p = nullptr;
    size_t cap = 0;  // elements
    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    Buffer(Buffer &&o) noexcept { *this = std::move(o); }
    Buffer &operator=(Buffer &&o) noexcept {  // (by exchange: what this one held goes with `o`)
        std::swap(p, o.p), std::swap(cap, o.cap);
        return *this;
    }
    ~Buffer() { release(); }
    operator T *() const { return p; }
    T *get() const { return p; }
    bool holds(size_t n) const { return cap >= n; }
    int ensure(size_t n) { return cap >= n ? (int) AWPU_OK : grow(n); }
    int grow(size_t n) {  // (ensure() decides; a caller with something to do before the old pointer goes asks holds() and comes here)
        release();
        const hipError_t e = Mem::alloc(reinterpret_cast<void **>(&p), n * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return hip_fail(e, Mem::what);
        }
        cap = n;
        return AWPU_OK;
    }
    void release() {
        if (p) Mem::free(p);
        p = nullptr, cap = 0;
    }
};
template <class T>
using DeviceBuffer = Buffer<T, DeviceMem>;
template <class T>
using PinnedBuffer = Buffer<T, PinnedMem<hipHostMallocDefault>>;
template <class T>
using PortablePinnedBuffer = Buffer<T, PinnedMem<hipHostMallocPortable>>;  // pinned for every device (a group's staging)

// a stream to wait for, and the device it belongs to
struct StreamOn {
    int device;
    hipStream_t stream;
};

// Two buffers for work that alternates between them, with which of them have been used since they were allocated and whose
// turn it is.  replace(): a pair that is too small (holds()) is replaced behind a synchronize of everybody who may still read it -- the
// caller says who -- each on its own device, and allocated on `device`; the used flags start again, the turn goes on (every
// reuse of a buffer waits for its last reader's event whatever the turn).  A failed allocation leaves cap() 0.
template <class Buf>
struct DoubleBuffer {
    Buf b[2];
    bool used[2] = {false, false};
    unsigned turn = 0;
    auto operator[](int k) const { return b[k].get(); }
    size_t cap() const { return b[1].cap; }  // (of each; b[1] is allocated last)
    bool holds(size_t n) const { return b[1].cap >= n; }
    int next() { return (int) (turn++ & 1); }
    template <class Readers>
    int replace(size_t n, int device, const Readers &readers) {
        for (const StreamOn &r : readers) {
            AWPU_HIP_TRY(hipSetDevice(r.device));
            AWPU_HIP_TRY(hipStreamSynchronize(r.stream));
        }
        AWPU_HIP_TRY(hipSetDevice(device));
        b[0].release(), b[1].release();
        used[0] = used[1] = false;
        if (const int rc = b[0].grow(n); rc != AWPU_OK) return rc;
        return b[1].grow(n);
    }
};

// Two buffers of `cap` bytes each for the two pieces a run has in flight (piece i uses [i & 1]): device memory, pinned host
// memory, or both.  Grow-only; what it held it keeps, at the new size; a failed allocation leaves cap 0.
struct BufferPair {
    DeviceBuffer<unsigned char> d[2];
    PinnedBuffer<unsigned char> h[2];
    size_t cap = 0;
    int ensure(size_t bytes, bool want_host, bool want_device = true) {
        if (bytes == 0 || (cap >= bytes && (h[0] || !want_host) && (d[0] || !want_device))) return AWPU_OK;
        want_host |= h[0] != nullptr;
        want_device |= d[0] != nullptr;
        bytes = std::max(bytes, cap);
        cap = 0;
        for (int b = 0; b < 2; b++) d[b].release(), h[b].release();
        for (int b = 0; b < 2; b++) {
            if (const int rc = want_device ? d[b].grow(bytes) : (int) AWPU_OK; rc != AWPU_OK) return rc;
            if (const int rc = want_host ? h[b].grow(bytes) : (int) AWPU_OK; rc != AWPU_OK) return rc;
        }
        cap = bytes;
        return AWPU_OK;
    }
};

// An event / a stream created at first ensure() and destroyed with its owner.  No timing unless asked to; `what` names a failure.
template <class H, hipError_t (*Destroy)(H)>
struct Owned {
    H it = nullptr;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() {
        if (it) (void) Destroy(it);
    }
    operator H() const { return it; }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    int ensure(unsigned flags = hipEventDisableTiming, const char *what = "hipEventCreateWithFlags") {
        if (it) return AWPU_OK;
        const hipError_t e = hipEventCreateWithFlags(&it, flags);
        return e == hipSuccess ? (int) AWPU_OK : hip_fail(e, what);
    }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    int ensure(const char *what = "hipStreamCreateWithFlags") {
        if (it) return AWPU_OK;
        const hipError_t e = hipStreamCreateWithFlags(&it, hipStreamNonBlocking);
        return e == hipSuccess ? (int) AWPU_OK : hip_fail(e, what);
    }
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
    DeviceBuffer<awpu::QuadEntry> d;
    size_t entries = 0;  // allocated (the launchers check their kernel's reach against it: das_kernels.h, Extents)
    awpu::FastPlan plan{};  // set by prepare() where the window fits the layout's image
};

// ---- the device group (awpu_group.cpp): what the group's handle owns, and what each of its parts owns as a member

// how a part of a group reaches devices[0]: kPeerSame (the same GPU), kPeerDirect (peer copies over xGMI) or
// kPeerStaged (no peer access on this node: the window and the tiles cross pinned host memory, explicitly)
enum PeerPath { kPeerSame = 0, kPeerDirect = 1, kPeerStaged = 2 };

// cfg.n_devices > 1: the handle owns no sweep state of its own, only one part (an ordinary single-device engine) per device
struct Group {
    std::vector<awpu_hip *> parts;
    bool union_window_done = false;  // every part stages the union of the parts' windows (packed frames need one layout)
    Event ev_fan;                    // recorded on the caller's stream, awaited by every part
    DoubleBuffer<DeviceBuffer<float>> packed;  // the packed frame pairs of a call on devices[0], sized for cfg.max_batch
    // pinned staging of what the staged parts get, sized for cfg.max_batch: the packed pairs, or the union of the parts' windows
    // of every stream (which of them, and where the window starts, is the call's: Payload in awpu_group.cpp).  ev_staged[b]: it is there
    DoubleBuffer<PortablePinnedBuffer<float>> stage;
    Event ev_staged[2];
};

// a part's share of the fan-out (awpu_hip_process_device on a group).  Two receive buffers, so that the copy of call k+1 (on the
// part's copy_stream) runs beside the sweep of call k (on its stream); the events that order them are the handle's ev_copied[]
// (shared with the host batches' pieces) and ev_swept[] here
struct GroupMember {
    // the part's pixels inside the group's range: (first pixel relative to the group's pixel_begin, count), ascending; the part's
    // own table and power rows hold them back to back.  One range = a contiguous slab; several = row groups of four dealt
    // round-robin over the devices (edge rows of the sine-space grid cost the quad shapes more than centre rows: DESIGN.md 6)
    std::vector<std::pair<int, int>> ranges;
    PeerPath peer = kPeerSame;
    DoubleBuffer<DeviceBuffer<float>> recv;
    Event ev_swept[2], ev_done;
    // staged parts only.  stage_used[b] / ev_staged_read[b]: its upload out of the group's stage[b] was enqueued / is done;
    // tile: pinned staging of its power tile on the way back; ev_tile_free[b]: the caller's stream has read tile[b]
    bool stage_used[2] = {false, false};
    Event ev_staged_read[2];
    DoubleBuffer<PortablePinnedBuffer<float>> tile;
    Event ev_tile_free[2];
};

}  // namespace awpu::host

struct awpu_hip {
    template <class T>
    using Dev = awpu::host::DeviceBuffer<T>;
    template <class T>
    using Pinned = awpu::host::PinnedBuffer<T>;
    using Event = awpu::host::Event;
    using Stream = awpu::host::Stream;

    awpu_hip_cfg cfg{};
    Stream stream;
    Event ev_begin, ev_end;  // the only two events that carry timing: recorded where a call asks for it (SweepOpts::timed)

    // host copies of what the reference keeps in MIMOWorker / Antenna
    std::vector<int32_t> off;   // [pixel_count][lut_stride]  offsetDelays
    std::vector<float> frac;    // [pixel_count][lut_stride]  fractionalDelays
    std::vector<int32_t> index; // [usable]                   antenna.index
    std::vector<float> gain;    // [n_streams] optional per-mic gain (awpu_hip_set_mic_gains); empty = none
    bool have_table = false, have_mics = false, prepared = false;

    // device state
    Dev<awpu::LutEntry> d_lut;
    struct FastLut {
        awpu::FastPlan plan;
        Dev<awpu::FastEntry> d;
        size_t entries = 0;  // allocated (the launchers check their kernel's reach against it: das_kernels.h, Extents)
    };
    std::vector<FastLut> fast_luts;  // one per (frames per item, LDS image size) in use
    Dev<awpu::FastEntry> d_exact_pair_lut;  // reference-order sweep on the frame-pair layout (das_exact_pair_kernel)
    size_t exact_pair_lut_entries = 0, fir_plane_lut_entries = 0;  // allocated entries of the table above and of the FIR8 plane table
    awpu::FastPlan exact_plan{};                  // ... its plan, and that of quad_tables[kQuadExact]
    awpu::host::QuadTable quad_tables[awpu::host::kQuadLayouts];  // the quad-major tables, by QuadLayout
    Dev<unsigned> d_nd_queue;                     // das_exact_nd_kernel's eight item counters (one per XCD)
    Dev<int2> d_nd_items;                         // ... and its item list (nd_items_kernel), valid for nd_items_key
    Dev<unsigned> d_nd_starts;                    // ... and its tiles' start table (build_quad_lut(kQuadExactNd): nd_tile_window.h), bytes
    size_t nd_start_entries = 0;
    long long nd_items_key = -1;                  // (n_pairs, pair group, quads per wave) the list was built for; -1: none
    int n_cus = 0;                                // compute units of the handle's device (persistent workgroups: one per CU)
    bool exact_nd_ok = false;     // ... and the window fits the {next, d} image (kQuadExactNd)
    // single frames: ... its halves form, chunked / every mic resident; fast_ndp_ok: AWPU_MATH_F32_FAST takes the chunked one on small grids
    bool exact_ndh_ok = false, exact_ndhs_ok = false, fast_ndp_ok = false;
    bool identity_mics = false;   // the active-mic list is 0 .. usable-1 (awpu_hip_set_active_mics(NULL)): rows need no look-up
    bool exact_pairs_ok = false;  // AWPU_MATH_F32_EXACT + LERP and the window fits the pair image
    Dev<uint32_t> d_fir_plane_lut;             // FIR8 on the four-plane layout: one dword per (pixel, mic): address, plane, coefficient row
    awpu::FastPlan fir_plane_plan{};
    bool fir_planes_ok = false;                // AWPU_MATH_F32_FAST + FIR8 and the window fits the plane image
    std::vector<float> fir;                    // host copy of the [101][8] coefficient table (baked into the plane entries)
    bool quadh_fits = false;      // single frames on the halves layout (das_quadh_kernel)
    bool quadhs_fits = false;     // ... with every active mic's row in LDS at once (das_quadh_stationary_kernel: one 8x8 array does)
    bool quad_ok = false;         // the table's statistics favour the quad shape (decided in prepare)
    double quad_cost = 0.0;       // its expected packed VALU instructions per quad and mic (32 = no sharing at all)
    double quad_differ = 3.0;     // pixels of a vertical quad (of three) whose integer delay differs from the second pixel's, per mic (table sample)
    Dev<int32_t> d_index;
    Dev<float> d_gain;   // [usable] gains in active-mic order, or null
    Dev<float> d_calib;  // [64] per-mic mean squares (calibration)
    Dev<awpu::LutEntry> d_beam_lut;  // [directions][usable] entries of awpu_hip_beams
    Dev<float> d_beam_out;           // [n] powers then [n][256] beams, n = d_beam_out.cap / 257: the directions it was allocated for
    // particle tracking (awpu_hip_track.h)
    std::vector<float> antenna;            // [3][antenna_n] element positions by stream id (awpu_hip_set_antenna); empty = none
    Dev<float> d_xyz;                      // ... on the device
    std::vector<int32_t> track_index;      // the active mics d_track_index holds
    Dev<int32_t> d_track_index;
    Dev<unsigned char> d_track;            // particles, then the reference used, then [n][256] beams (steer_table_device: angles, tables)
    Dev<float> d_fir;                   // [101][8] coefficient table (AWPU_INTERP_FIR8)
    Dev<float> d_ring;                  // [n_streams][2048] history ring (awpu_hip_ingest_block)
    Dev<uint8_t> d_display;             // awpu_hip_live_block: peak (one float), compact image, upscaled image
    Dev<awpu::ResizeTap> d_taps;        // column + row taps of the display upscale, for taps_key
    int taps_key[4] = {0, 0, 0, 0};     // {srows, scols, drows, dcols}
    int taps_band_rows = 0;             // ... and the most compact rows a 16-row tile of the large image reads (watch_kernels.h)
    Dev<float> d_pack;                  // [pairs][usable][wp][2] sample-interleaved frame pairs
    Dev<unsigned char> d_datagrams;     // staging for one block of wire datagrams
    Dev<int32_t> d_row_off_ring;        // row offsets for frames read out of the ring (pitch 2048)
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
    Dev<int32_t> d_row_off;
    Dev<int32_t> d_row_off_compact;        // the same for frames uploaded as [streams][compact_hist] windows
    int compact_hist = 0;                  // 0 = the window cannot be cut out (it touches the newest sample)
    Dev<float> d_frames;
    Pinned<float> h_live_in, h_live_out;                // pinned staging of awpu_hip_process's one-frame calls (the live path): window in, powers out
    unsigned live_calls = 0;                            // ... how many of them this handle has served (every 32nd is timed by events)
    // ... their completion flag (the resident single-frame kernels with one quad per wave): the device counter the workgroups count themselves on, what it will read
    // when every launch armed so far is over, the pinned flag and the sequence number of the last armed launch.  (Whether a launch
    // is armed is the call's: SweepOpts::flag)
    Dev<unsigned long long> d_done_counter;
    unsigned long long done_total = 0;
    Pinned<unsigned> h_done_flag;
    unsigned done_seq = 0;
    Dev<float> d_power;
    int wstart = 0, window = 0, tau_max = 0;
    int pair_cols = 0;  // frame-pair sweep: > 0 = waves take vertically adjacent pixels (grid row length), 0 = consecutive

    // device group (awpu_group.cpp): `group` is empty unless cfg.n_devices > 1, `member` unless the handle is a part of one
    awpu::host::Group group;
    awpu::host::GroupMember member;
    // a second stream for uploads that run beside the sweeps, and "upload b is over": shared by the pieces of a host batch
    // (enqueue_host_process), the runs of blocks (run_pieces.cpp) and a part's receive buffers, which is why they live here
    // and not in `member`.  Created at first use; a part's at its creation
    Stream copy_stream;
    Event ev_copied[2];
    bool in_flight = false;                 // awpu_hip_process_async without its awpu_hip_wait yet
    // call order across streams (awpu_hip.h, "Streams" (c); enter_stream below): the stream the handle's last call enqueued its
    // work on -- the handle's own from creation and after awpu_hip_synchronize; a group's: its first part's, there -- and the
    // event that takes the next call's stream behind it where that is another stream
    hipStream_t last_stream = nullptr;
    Event ev_order;
    // runs of blocks (run_pieces.cpp), by piece: piece i's history [n_streams][768 + 256 * piece] in blk_hist.d[i & 1], its windows
    // in d_blk_frames; the host forms stage piece i's input in pinned blk_in.h[i & 1], upload it to blk_in.d[i & 1] on copy_stream
    // and bring its powers back through pinned blk_out.h[i & 1]
    awpu::host::BufferPair blk_hist, blk_in, blk_out;
    Dev<float> d_blk_frames;
    // ev_blk_in[b]: blk_in.h[b] may be refilled; ev_blk_hist[b]: blk_hist.d[b] formed; ev_blk_cut[b]: ... and read by the cut;
    // ev_blk_swept[b]: d_power's half b holds its piece's powers; ev_blk_out[b]: ... and blk_out.h[b] too; ev_blk_ring: orders a
    // run after the work queued on the handle's stream, and the handle's stream after a device-form run on the caller's stream
    Event ev_blk_in[2], ev_blk_hist[2], ev_blk_cut[2], ev_blk_swept[2], ev_blk_out[2], ev_blk_ring;
    // listening to such runs (awpu_hip_listen.h): the listeners on the device from piece to piece; the host forms get piece i's
    // audio rows [n][256 * piece], then its trail, in listen_out.d[i & 1] and bring them back through pinned listen_out.h[i & 1].
    // listen_stream: where the listen kernels run beside the sweeps when heatmaps are asked for too.
    Dev<unsigned char> d_listeners;
    awpu::host::BufferPair listen_out;
    Stream listen_stream;
    // ev_listened[b]: the listen kernels have read blk_hist.d[b] (and written listen_out.d[b]); ev_listen_out[b]: listen_out.h[b] holds it
    Event ev_listened[2], ev_listen_out[2];

    // watching such runs (awpu_hip_watch.h), exposed and coherence runs alike: piece i's peaks, compact images and (host forms)
    // large images in watch.d[i & 1]; the host forms bring the images back through pinned watch.h[i & 1].  Laid out by the display
    // step alone (struct Display in watch_run.h).  The events are those of the runs above: ev_blk_swept[b] is recorded behind the
    // display kernels, ev_blk_out[b] behind the images' way back.
    awpu::host::BufferPair watch;
    // finding in such runs (awpu_hip_find.h), host forms: piece i's counts, then its sources, in find_out.d[i & 1] and back through
    // pinned find_out.h[i & 1], behind the same two events; locating (awpu_hip_focus.h) adds its ranges and the candidates' powers
    // behind them (the device form: only the powers nobody asked for, in find_out.d[0]).  Laid out by the display step as well.
    awpu::host::BufferPair find_out;
    // exposing such runs (awpu_hip_expose.h): the open window's row [pixel_count] from piece to piece and from the caller's `carry`
    // to it, and the frames that close inside piece i in expose.d[i & 1] (the device form: in expose.d[0], where nobody asked for
    // them).  The host forms bring them back through pinned blk_out.h[i & 1], which an exposed run's swept powers never cross
    Dev<float> d_expose_carry;
    awpu::host::BufferPair expose;
    // coherence (awpu_hip_cohere.h): the sweep's table where prepare() builds no d_lut (AWPU_MATH_F32_FAST: ensure_cohere_table; freed
    // with the other tables), and the maps of a host-form call on their way back, one plane [batch][pixel_count] per map asked for
    Dev<awpu::LutEntry> d_cohere_lut;
    Dev<float> d_cohere_out;
    // tones (awpu_hip_tones.h): the rule's tables as the host functions make them -- the two windows [2][256], then the twiddles
    // [128][2] --, uploaded once per handle (ensure_tones_tables), and the planes of a host-form call on their way back: tone
    // [batch][n_groups][pixel_count], then pitch [batch][pixel_count]
    Dev<float> d_tones_tables;
    Dev<float> d_tones_out;
    // cross-spectral maps (awpu_hip_csm.h; awpu_csm.cpp): the spectra of the blocks being accumulated where the caller keeps none,
    // and what a host-form call brings up and back (samples or a matrix in, the matrix or the planes out)
    Dev<float> d_csm_spectra, d_csm_io;
    // ... and the loaded inverse's scratch (awpu_csm.cpp; csm_invert_kernels.h): the factor L and its inverse M in double,
    // [n_bins][usable][usable][2] each, then the bins' state words
    Dev<double> d_csm_invert;
    // ... and the eigendecomposition's (awpu_hip_csm_eig.h; awpu_csm_eig.cpp): the Jacobi kernel's scratch in double
    // (csm_eig_kernels.h lays it out), and what a subspace map keeps between its steps: the vectors and the weighed matrix
    // [n_bins][usable][usable][2] each, q [n_bins][pixel_count], then the values [n_bins][usable] and the solved words [n_bins]
    // where the caller keeps none
    Dev<double> d_csm_eig;
    Dev<float> d_csm_eig_rows;
    // ... and a cross-spectral run's (awpu_hip_csm_watch.h): the spectra store, the carry, one frame's matrix and inverse, a piece's
    // rows, planes, solved words and step records, a chunk's samples and datagrams (csm_run_plan.h lays it out)
    Dev<float> d_csm_run;
    // ... and CLEAN-SC's (awpu_hip_csm_clean.h; awpu_csm_clean.cpp): the working matrix D [n_bins][usable][usable][2] where the
    // caller keeps none; the component v [n_bins][usable][2], then the loop's dirty planes [n_bins][pixel_count]; the bins'
    // bookkeeping (CsmCleanState [8]); and what a host-form call brings up and back (the matrix in, D, the steps and three planes out)
    Dev<float> d_csm_clean_matrix, d_csm_clean_rows;
    Dev<unsigned char> d_csm_clean_state, d_csm_clean_io;
    // peeling (awpu_hip_peel.h; awpu_peel.cpp): the table's reach at the active mics, valid for the tables of peel_gen (table_gen;
    // 0: none yet); the loop's residual frames [batch][n_streams][hist] where the caller keeps none, its power row P_k
    // [batch][pixel_count], its bookkeeping (PeelState [batch]), and the results of a host-form call on their way back
    int peel_min_off = 0, peel_max_off = 0;
    unsigned long long peel_gen = 0;
    Dev<float> d_peel_frames, d_peel_power;
    Dev<unsigned char> d_peel_state, d_peel_out;
    awpu::host::BufferPair peel_steps;  // peel runs, host forms: piece i's steps in peel_steps.d[i & 1], back through pinned .h[i & 1]

    // the band (awpu_hip_band.h): its coefficients (empty = none; they travel to the pre-pass as kernel arguments), and the
    // filtered frames of a call whose own frames are the caller's or the ring's, in those frames' layout (band_sweep): a plane
    // per band, where a spectral call (awpu_hip_spectral.h) brings several
    std::vector<float> band;
    Dev<float> d_band;
    int band_taps() const { return static_cast<int>(band.size()); }
    // spectral runs (awpu_hip_spectral.h), by piece as `watch`: every frame's band maxima, its three-byte image, its dominant
    // bands and (host forms) its large image
    awpu::host::BufferPair spectral;

    awpu_hip_stats stats{};
    std::string last_error;                  // awpu_hip_last_error_of
    Dev<unsigned long long> d_diag;          // AWPU_FAST_DEBUG=16 cycle stamps of the last launch

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
// what sweeps AWPU_MATH_F32_EXACT (AWPU_SHAPE=exact_*; the values are those AWPU_EXACT_PAIRS=<n> of a tuning build takes)
enum class ExactShape : int {
    kVerify = 0,   // the round-1 verification kernel (das_exact_kernel)
    kDefault = 1,  // launch()'s rule
    kPair = 2,     // the two-pixel reference-order block even where quads would run
    kQuad = 3,     // round 4's quad kernel on raw sample pairs (cur - next per pixel)
    kNd1 = 4,      // the {next, d} kernel with one quad per wave
    kNd2 = 5,      // ... with two
    kNdp = 6,      // single frames: one pixel per wave (das_exact_ndp_kernel) wherever its rows can be chunked
};
inline bool forces_exact_nd(ExactShape e) { return e == ExactShape::kNd1 || e == ExactShape::kNd2 || e == ExactShape::kNdp; }

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
    ExactShape exact_pairs = ExactShape::kDefault;
    int pair_cols = -1;            // 0 / 1: the pair shape pairs consecutive / vertically adjacent pixels (default: whichever coincides more)
    int group_copy = 0;            // AWPU_GROUP_FORCE_COPY
    int listen_stream = 1;         // tuning: 0 = the listen kernels queue behind the sweeps instead of running beside them
    EnvKnobs();
};
const EnvKnobs &env();

// The bands in front of a sweep: none, the handle's own (awpu_hip_band.h) or those of a spectral call (awpu_hip_spectral.h).  The
// coefficients stay their owner's: a set lives no longer than the call that made it.
struct BandSet {
    int n = 0;
    int taps[AWPU_SPECTRAL_MAX_BANDS] = {0, 0, 0, 0};
    const float *coef[AWPU_SPECTRAL_MAX_BANDS] = {nullptr, nullptr, nullptr, nullptr};
    int max_taps() const { return std::max(std::max(taps[0], taps[1]), std::max(taps[2], taps[3])); }
    int planes() const { return std::max(n, 1); }  // what a sweep's windows and powers are held in
};
inline BandSet own_band(const awpu_hip *h) {
    BandSet set;
    if (!h->band.empty()) set.n = 1, set.taps[0] = h->band_taps(), set.coef[0] = h->band.data();
    return set;
}

// layout of d_frames: kFull [batch][n_streams][hist]; kCompact [batch][n_streams][compact_hist] with
// sample 0 = history sample wstart; kRing one frame read in place from the ingest ring (rows 2048 apart)
enum FrameLayout { kFull = 0, kCompact = 1, kRing = 2 };

// What a sweep is asked besides its frames: arguments of the call in progress, handed down from the ABI function that starts it and
// never kept in the handle.  The default is every asynchronous path's: the caller times its own stream ("Who records the
// event bracket").
struct SweepOpts {
    bool timed = false;     // record ev_begin in front of the launch's first kernel, ev_end behind its last
    float *sums = nullptr;  // awpu_hip_process_device_sums: where out[] goes
    bool *flag = nullptr;   // live_host_call: non-null = raise the completion flag where the kernel can; *flag = it will
};
inline constexpr SweepOpts kTimed{true};
// One sweep as its launcher sees it (awpu_sweep.cpp): built once in launch() and once in sweep_packed()
struct SweepCall {
    const float *frames;       // in `layout`; null: the caller's packed pairs
    int batch;
    float *power;
    hipStream_t stream;
    int layout;                // FrameLayout
    int hist_eff, wstart_eff;  // floats between two streams of a frame, and where the window starts in such a row
    SweepOpts opts;
    int hist_ring() const { return layout == kRing ? AWPU_HIST : hist_eff; }  // the history a stream offers a filter (the ring's rows are 2048 floats apart)
};

// the sweep layer: defined, and described, in awpu_sweep.cpp
int prepare(awpu_hip *h);
void free_tables(awpu_hip *h);
int launch(awpu_hip *h, const float *d_frames, int batch, float *d_power, hipStream_t s, int layout = kFull, const SweepOpts &o = {});
// what a coherence sweep (awpu_hip_cohere.h) writes, device memory, each or null: the three maps [batch][pixel_count], out[] and
// e[] of every pixel [batch][pixel_count][256]
struct CohereOut {
    float *power = nullptr, *coherence = nullptr, *weighted = nullptr, *sums = nullptr, *energy = nullptr;
};
int ensure_cohere_table(awpu_hip *h);  // behind check_ready, before the call enqueues anything: the one step that may block
int launch_cohere(awpu_hip *h, const float *d_frames, int batch, const CohereOut &out, hipStream_t s, int layout, bool timed = false);
// what a tone sweep (awpu_hip_tones.h) writes, device memory, each or null: tone [batch][n_groups][pixel_count], pitch and
// pitch_row = (float) pitch [batch][pixel_count], bins [batch][pixel_count][129], spectrum [batch][pixel_count][129][2]
struct TonesOut {
    float *tone = nullptr;
    int32_t *pitch = nullptr;
    float *pitch_row = nullptr, *bins = nullptr, *spectrum = nullptr;
};
int ensure_tones_tables(awpu_hip *h);  // beside ensure_cohere_table: may block, before the call enqueues anything
int launch_tones(awpu_hip *h, const float *d_frames, int batch, const awpu_tones_t &t, const TonesOut &out, hipStream_t s, int layout, bool timed = false);
bool takes_packed_pairs(awpu_hip *h, int batch, awpu::FastPlan *plan);
int packed_shape(awpu_hip *h, int batch, awpu::FastPlan *plan);
size_t packed_floats_of(const awpu_hip *h, const awpu::FastPlan &plan, int batch);
int pack_for_sweep(awpu_hip *h, const awpu::FastPlan &plan, const float *d_frames, int batch, float *d_packed, hipStream_t s);
int sweep_packed(awpu_hip *h, const awpu::FastPlan &plan, const float *d_packed, size_t packed_floats, int batch, float *d_power, hipStream_t s);  // (untimed)

// defined, and described, in awpu_hip.cpp
void retire_live_graphs(awpu_hip *h);
int enqueue_host_process(awpu_hip *h, const float *frames, int batch, const BandSet *bands = nullptr);  // (null: the handle's own band, if any)
int enqueue_power_to_host(awpu_hip *h, int batch, float *power, size_t pitch);
int enqueue_ingest(awpu_hip *h, const void *datagrams, int32_t stride_bytes);
int check_ready(awpu_hip *h, int batch);
int enter_stream(awpu_hip *h, hipStream_t s);  // the call that is about to enqueue on `s`, behind the handle's last call
inline hipStream_t stream_of(const awpu_hip *h, void *stream) { return stream ? static_cast<hipStream_t>(stream) : (hipStream_t) h->stream; }
extern const char *const kBandHistory;  // what AWPU_ERR_RANGE says where the bands' history does not fit a snapshot
int ensure_power(awpu_hip *h, size_t need_power);
int ensure_ring(awpu_hip *h);
int host_piece(int batch);
int wait_and_time(awpu_hip *h, bool timed);
size_t align16(size_t n);
int check_particles(const awpu_particle_t *p, int32_t n, double theta_limit, double reference);
int check_antenna(const awpu_hip *h);
int ensure_track_index(awpu_hip *h);
int check_candidates(const double *distance, int32_t n_dist);  // awpu_focus.cpp: the candidate distances of awpu_hip_focus.h
int ensure_taps(awpu_hip *h, int rows, int cols, int out_rows, int out_cols, hipStream_t s);
// a sweep of its own behind band_sweep's pre-pass, in place of launch() (the coherence sweep, the tone sweep): the frames in the
// call's layout and whether to time it -> status
using OwnSweep = std::function<int(const float *d_frames, bool timed)>;
int band_cut(awpu_hip *h, const BandSet &bands, const float *in, long long in_frame, long long in_row, int in_lo, int batch, float *out,
             long long out_plane, int layout, hipStream_t s);
int band_sweep(awpu_hip *h, const BandSet &bands, const float *in, long long in_frame, long long in_row, int in_lo, int batch, float *d_power,
               long long power_plane, hipStream_t s, int layout, const SweepOpts &o = {}, const OwnSweep *own = nullptr);
inline int band_sweep(awpu_hip *h, const float *in, long long in_frame, long long in_row, int in_lo, int batch, float *d_power, hipStream_t s, int layout,
                      const SweepOpts &o = {}) {
    return band_sweep(h, own_band(h), in, in_frame, in_row, in_lo, batch, d_power, 0, s, layout, o);  // the handle's own band: the one-band case
}

// A buffer whose pointer the captured live-block graphs bake in (d_power, d_pack, d_display): they are retired before the old pointer
// goes.  (prepare() and ensure_taps() retire for the tables and d_taps; launch_exact_nd for d_nd_items, a synchronize before it grows.)
template <class B>
int ensure_seen_by_live_graphs(awpu_hip *h, B &buf, size_t n) {
    if (buf.holds(n)) return AWPU_OK;
    retire_live_graphs(h);
    return buf.grow(n);
}

// the device group: defined, and described, in awpu_group.cpp.  The ABI functions hand a group's handle over to these
inline bool is_group(const awpu_hip *h) { return !h->group.parts.empty(); }
// calls that are not pixel-sharded: a device group answers with its first device
inline awpu_hip *first_device(awpu_hip *h) { return h && is_group(h) ? h->group.parts[0] : h; }
int create_group(awpu_hip_t **out, const awpu_hip_cfg &c);
int group_set_delay_table(awpu_hip *g, const int32_t *off, const float *frac);
int group_set_active_mics(awpu_hip *g, const int32_t *index, int32_t usable);
int group_set_mic_gains(awpu_hip *g, const float *gains);
int group_set_fir_table(awpu_hip *g, const float *coeffs);
int group_process(awpu_hip *g, const float *frames, int batch, float *power);
int group_process_async(awpu_hip *g, const float *frames, int batch, float *power);
int group_wait(awpu_hip *g);
int group_process_device(awpu_hip *g, const float *d_frames, int batch, float *d_power, hipStream_t stream);
int group_enter_host(awpu_hip *g);  // enter_stream for a group's host-form calls, which enqueue on the parts' own streams
int group_ingest_block(awpu_hip *g, const void *datagrams, int32_t stride_bytes);
int group_process_ring(awpu_hip *g, float *power);
int group_synchronize(awpu_hip *g);
int group_peer_status(awpu_hip *g, int32_t *status, int32_t n);
int group_stats(awpu_hip *g, awpu_hip_stats *out);
}  // namespace awpu::host
