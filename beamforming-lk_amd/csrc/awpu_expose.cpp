// awpu_expose.cpp -- the handle forms of include/awpu_hip_expose.h: awpu_hip_expose_rows_device and the exposed runs of blocks.
// The rule is expose_rule.h's, the kernels expose_kernels.hip's; what an exposed frame shows goes through the watch run's
// display step (watch_run.h); awpu_hip_expose_rows is expose_host.cpp's.
#include "watch_run.h"

#include "awpu_hip_expose.h"
#include "expose_kernels.h"

using namespace awpu::host;

namespace {

// ---- exposure (awpu_hip_expose.h; kernels in expose_kernels.hip) -----------------------------------------------------------------
// The items of an exposed run are its SWEPT blocks, in order: the blocks of every window that lie inside the call, the skipped
// ones between the windows left out.  With c = carry_in, item s is block q = (s + c) % L of window j = (s + c) / L, and (s + c) / L
// frames close in front of it.  A piece is n consecutive items, and its history holds only the blocks their snapshots read, by the
// slot map of expose_kernels.h: formed like a watch piece's, blocks from before the call out of the ring's snapshot, the rest
// staged and uploaded (host forms) or gathered out of the caller's samples (device form).  The windows are cut a window's items at
// a launch (consecutive blocks: launch_watch_cut, or the band's pre-pass, with a step of one block); where every == length the
// whole piece is one.  Behind the piece's sweep comes launch_expose on its powers -- the open window arrives and leaves in
// d_expose_carry --, and behind that the display step and the peak pass of a watch run on the frames that closed inside the
// piece.  Their number varies from piece to piece, so exposed powers, images and sources all travel through show / fetch_shown /
// deliver_shown and Consumer::power stays null.  The ring's new snapshot: as in a watch run.

struct ExposeRun {
    WatchRun shown;          // what it shows and where to: the outputs and the find request of a watch run, for the exposed frames
    awpu_expose_t e{};
    awpu::ExposeCount n{};
    float *carry = nullptr;  // host memory in the host forms, device memory in the device form, like the outputs
};

struct ExposePieces final : Consumer {
    awpu_hip *const h;
    const BlockRun &src;
    const ExposeRun &er;
    const awpu_watch_t &w;
    const bool host;
    const int S, L, E, c_in;
    const size_t P;
    Display display;
    float *const exposed;               // the exposed frames' powers, or null (Consumer::power, the swept blocks', stays null)
    int lo = 0, width = 0;
    const float *snapshot = nullptr;    // blocks -4 .. -1 of the call
    hipStream_t sw = nullptr;
    std::vector<float> carried;         // host forms: the open window after the run

    ExposePieces(awpu_hip *h_, const BlockRun &src_, int n_blocks_, const ExposeRun &er_)
        : h(h_), src(src_), er(er_), w(er_.shown.w), host(!src_.device), S(h_->cfg.n_streams), L(er_.e.length), E(er_.shown.w.every),
          c_in(er_.n.carry_in), P((size_t) h_->cfg.pixel_count), display(h_, er_.shown, !src_.device), exposed(er_.shown.power) {
        n_items = er.n.n_swept;
        n_blocks = n_blocks_;
        // the last block of the call swept: the ring's new snapshot is the tail of the last piece's history
        tail = n_items == 0 || item_block(n_items - 1) != n_blocks - 1;
    }
    int item_block(int s) const { return w.first + (s + c_in) / L * E - (L - 1) + (s + c_in) % L; }
    int frames_before(int s) const { return (s + c_in) / L; }
    int closed_in(const Piece &p) const { return frames_before(p.first + p.n) - frames_before(p.first); }  // the frames a piece shows
    // the slot map of a piece's history
    awpu::ExposeSlots map(const Piece &p) const {
        if (p.tail) return {n_blocks - 1, 1, n_blocks - 1 + E, E, L, false};
        const int q0 = (p.first + c_in) % L, k0 = item_block(p.first);
        return {k0, std::min(p.n, L - q0), k0 - q0 + E, E, L, E - L >= 3};
    }
    static int slots_of(const Piece &p, const awpu::ExposeSlots &m) { return m.slots(p.tail ? 1 : p.n); }
    // the most slots a piece of n items has: its items and, per window it touches, three blocks (own slots) or the gap (consecutive)
    int slots_max(int n) const {
        const int windows = (n + 2 * L - 2) / L;
        return E - L >= 3 ? n + 3 * windows : n + 3 + (windows - 1) * (E - L);
    }

    int check() override { return display.check(); }
    int ensure(int piece_max, int lo_, int width_, hipStream_t sw_) override {
        lo = lo_, width = width_, sw = sw_;
        const int most = std::max(slots_max(piece_max), 4);
        pitch = awpu::kSamples * most;
        snapshot = h->d_ring + h->ring_pos;
        int rc = ensure_run_buffers(h, src, piece_max, width, true, most - 3, most, bands.planes());
        if (rc == AWPU_OK && !host) rc = ensure_power(h, (size_t) piece_max * P * bands.planes());
        if (rc == AWPU_OK) rc = h->d_expose_carry.ensure(P);
        if (rc == AWPU_OK && (host || !exposed)) rc = h->expose.ensure((size_t) piece_max * P * sizeof(float), false);
        if (rc == AWPU_OK) rc = display.ensure(piece_max, sw);
        if (host && er.n.carry_out > 0) carried.resize(P);
        return rc;
    }
    int begin(hipStream_t s) override {
        if (c_in > 0)
            AWPU_HIP_TRY(hipMemcpyAsync(h->d_expose_carry, er.carry, P * sizeof(float), host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
        return AWPU_OK;
    }
    int staged_blocks(const Piece &p) override {
        const awpu::ExposeSlots m = map(p);
        const int slots = slots_of(p, m), q = std::max(0, 3 - m.k0);
        stage_slots(h, src, [&](int slot) { return m.slot_block(slot); }, q, slots, p.b);
        return slots - q;
    }
    int history(const Piece &p, hipStream_t s) override {
        const awpu::ExposeSlots m = map(p);
        return gathered_history(h, src, p.b, std::max(0, 3 - m.k0), slots_of(p, m), pitch, s, [&](const float *from, long long from_pitch, int n) {
            return awpu::launch_expose_gather(from, from_pitch, snapshot, m, S, hist_of(h, p.b), pitch, 0, n, s);
        });
    }
    int cut(const Piece &p, hipStream_t s) override {
        const awpu::ExposeSlots m = map(p);
        const size_t frame = (size_t) S * width;
        for (int i0 = 0, i1; i0 < p.n; i0 = i1) {  // items [i0, i1): consecutive blocks in consecutive slots
            i1 = E == L ? p.n : (i0 < m.n0 ? m.n0 : std::min(i0 + L, p.n));
            const float *from = hist_of(h, p.b) + (size_t) awpu::kSamples * m.item_slot(i0);
            float *to = h->d_blk_frames + i0 * frame;
            if (bands.n) {
                if (const int rc = band_cut(h, bands, from, awpu::kSamples, pitch, h->wstart, i1 - i0, to, (long long) frame * p.n, h->compact_hist > 0 ? kCompact : kFull, s)) return rc;
            } else {
                AWPU_HIP_TRY(awpu::launch_watch_cut(from, pitch, S, i1 - i0, awpu::kSamples, lo, width, to, s));
            }
        }
        return AWPU_OK;
    }
    int show(const Piece &p, float *d_pow, long long, hipStream_t s) override {
        const int j0 = frames_before(p.first);
        const awpu::ExposeWindows win{p.n, -((p.first + c_in) % L), L, L};
        float *d_frames = host || !exposed ?reinterpret_cast<float *>(h->expose.d[host ? p.b : 0].get()) : exposed + (size_t) j0 * P;
        AWPU_HIP_TRY(awpu::launch_expose(d_pow, (long long) P, win, er.e.mode, h->d_expose_carry, d_frames, s));  // (no frame closes: the carry still moves on)
        return display.show(p.b, j0, closed_in(p), d_frames, s);
    }
    int fetch_shown(const Piece &p, hipStream_t s) override {
        const int nf = closed_in(p);
        if (nf && exposed) AWPU_HIP_TRY(hipMemcpyAsync(h->blk_out.h[p.b], h->expose.d[p.b], (size_t) nf * P * sizeof(float), hipMemcpyDeviceToHost, s));
        return display.fetch(p.b, nf, s);
    }
    int deliver_shown(const Piece &p) override {
        const int j0 = frames_before(p.first), nf = closed_in(p);
        if (nf && exposed) std::memcpy(exposed + (size_t) j0 * P, h->blk_out.h[p.b], (size_t) nf * P * sizeof(float));
        return display.deliver(p.b, j0, nf);
    }
    int ring_from(const Piece &last) override { return awpu::kSamples * (slots_of(last, map(last)) - 4); }
    // the open window, behind the last piece's exposure on the sweep's stream (whatever stream the listen kernels of other runs have)
    int end(hipStream_t) override {
        if (er.n.carry_out == 0) return AWPU_OK;
        if (host)
            AWPU_HIP_TRY(hipMemcpyAsync(carried.data(), h->d_expose_carry, P * sizeof(float), hipMemcpyDeviceToHost, sw));
        else
            AWPU_HIP_TRY(hipMemcpyAsync(er.carry, h->d_expose_carry, P * sizeof(float), hipMemcpyDeviceToDevice, sw));
        return AWPU_OK;
    }
};

// the checks of an expose call that read no handle; then the run
int expose_run(awpu_hip *h, const BlockRun &src, int n_blocks, const awpu_watch_t *w, const awpu_expose_t *e, const awpu_find_t *f, float *carry,
               uint8_t *image, uint8_t *big, float *power, awpu_source_t *sources, int32_t *count, hipStream_t user) {
    ShownRun sr;
    if (const int rc = sr.open(w, n_blocks, [&] { return awpu::expose_refusal(e, w->every); }, f, image, big, power, sources, count)) return rc;
    const ExposeRun er{sr.wr, *e, awpu::expose_count(n_blocks, w->first, w->every, e->length), carry};
    if (!carry && (er.n.carry_in > 0 || er.n.carry_out > 0)) return invalid("null carry with a window open across the call's ends");
    AWPU_CTX(h);
    ExposePieces c(h, src, n_blocks, er);
    const int rc = run_pieces(h, src, user, c);
    if (rc == AWPU_OK && !src.device && er.n.carry_out > 0) std::memcpy(carry, c.carried.data(), c.carried.size() * sizeof(float));
    return rc;
}

}  // namespace

extern "C" {

int awpu_hip_expose_rows_device(awpu_hip_t *h, const float *d_power, int32_t n_blocks, int32_t n_pixels, int32_t first, int32_t every,
                                const awpu_expose_t *e, float *d_carry, float *d_frames, void *stream) {
    if (!h || !d_power) return invalid("null argument");
    if (n_blocks < 1 || n_pixels < 1 || first < 0 || every < 1) return invalid("n_blocks, n_pixels, every below 1 or first below 0");
    if (const char *why = awpu::expose_refusal(e, every)) return invalid(why);
    const awpu::ExposeCount n = awpu::expose_count(n_blocks, first, every, e->length);
    if (!d_carry && (n.carry_in > 0 || n.carry_out > 0)) return invalid("null carry with a window open across the call's ends");
    if (!d_frames && n.n_frames > 0) return invalid("null argument");
    h = first_device(h);
    AWPU_CTX(h);
    AWPU_HIP_TRY(hipSetDevice(h->cfg.device));
    const awpu::ExposeWindows win{n_blocks, first - (e->length - 1), every, e->length};
    AWPU_HIP_TRY(awpu::launch_expose(d_power, n_pixels, win, e->mode, d_carry, d_frames, stream_of(h, stream)));
    return AWPU_OK;
}

int awpu_hip_expose_blocks(awpu_hip_t *h, const void *datagrams, int32_t stride_bytes, int32_t n_blocks, const awpu_watch_t *w,
                           const awpu_expose_t *e, const awpu_find_t *f, float *carry, uint8_t *image, uint8_t *big_image, float *power,
                           awpu_source_t *sources, int32_t *count) {
    BlockRun src;
    if (int rc = wire_source(h, datagrams, stride_bytes, n_blocks, &src)) return rc;
    return expose_run(h, src, n_blocks, w, e, f, carry, image, big_image, power, sources, count, nullptr);
}

int awpu_hip_expose_samples(awpu_hip_t *h, const float *samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                            const awpu_expose_t *e, const awpu_find_t *f, float *carry, uint8_t *image, uint8_t *big_image, float *power,
                            awpu_source_t *sources, int32_t *count) {
    BlockRun src;
    if (int rc = sample_source(h, samples, pitch, n_blocks, false, &src)) return rc;
    return expose_run(h, src, n_blocks, w, e, f, carry, image, big_image, power, sources, count, nullptr);
}

int awpu_hip_expose_samples_device(awpu_hip_t *h, const float *d_samples, int64_t pitch, int32_t n_blocks, const awpu_watch_t *w,
                                   const awpu_expose_t *e, const awpu_find_t *f, float *d_carry, uint8_t *d_image, uint8_t *d_big_image,
                                   float *d_power, awpu_source_t *d_sources, int32_t *d_count, void *stream) {
    BlockRun src;
    if (int rc = sample_source(h, d_samples, pitch, n_blocks, true, &src)) return rc;
    return expose_run(h, src, n_blocks, w, e, f, d_carry, d_image, d_big_image, d_power, d_sources, d_count, static_cast<hipStream_t>(stream));
}

}  // extern "C"
