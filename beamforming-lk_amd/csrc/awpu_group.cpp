// awpu_group.cpp -- the device group of libawpu_hip.so (cfg.n_devices > 1): one handle, one part (an ordinary
// single-device engine) per GPU, each owning some of the handle's pixels.  Everything here runs in the caller's thread; the
// parts' streams run concurrently.  No collective library: host frames are uploaded by every device itself, device frames fan
// out from devices[0] by one peer copy per destination (a different xGMI link each).  The ABI functions (awpu_hip.cpp) hand a
// group's handle over to the group_ functions below; what a group and its parts own for this is Group / GroupMember
// (awpu_handle.h).
#include "awpu_handle.h"

#include <cstring>
#include <new>

using namespace awpu::host;

namespace {

// a part ran into an error: the group reports it as its own
int part_failed(awpu_hip *g, awpu_hip *part, int rc) {
    const std::string why = part->last_error.empty() ? std::string(awpu_hip_last_error()) : part->last_error;
    g->last_error = why;
    note_error(why);
    return rc;
}

template <class F>
int for_each_part(awpu_hip *g, F f) {
    for (awpu_hip *part : g->group.parts) {
        const int rc = f(part);
        if (rc != AWPU_OK) return part_failed(g, part, rc);
    }
    return AWPU_OK;
}

// the setters: the union window of the OLD table or mic list is void -- back to the caller's window, if any, and taken anew
void reset_union_window(awpu_hip *g) {
    g->group.union_window_done = false;
    for (awpu_hip *part : g->group.parts) {
        part->cfg.window_begin = g->cfg.window_begin;
        part->cfg.window_end = g->cfg.window_end;
    }
}

// host frames: every part uploads them itself and sends its pixels' powers into the caller's image
int enqueue_host_parts(awpu_hip *g, const float *frames, int batch, float *power) {
    if (const int rc = group_enter_host(g); rc != AWPU_OK) return rc;
    return for_each_part(g, [&](awpu_hip *part) {
        AWPU_CTX(part);
        const int r = enqueue_host_process(part, frames, batch);
        return r != AWPU_OK ? r : enqueue_power_to_host(part, batch, power, (size_t) g->cfg.pixel_count);
    });
}

}  // namespace

namespace awpu::host {

int create_group(awpu_hip_t **out, const awpu_hip_cfg &c) {
    if (c.n_devices > AWPU_MAX_DEVICES) return invalid("n_devices above AWPU_MAX_DEVICES");
    const int G = c.n_devices;
    // slabs: whole grid rows when the row length is known and the handle's range is whole rows, else pixels
    const bool by_rows = c.grid_columns > 0 && c.pixel_count % c.grid_columns == 0 && c.pixel_begin % c.grid_columns == 0;
    int unit = by_rows ? c.grid_columns : 1;
    // groups of four rows where that divides (the quad shapes sweep four rows at a time: slabs that start on a
    // multiple of four rows sweep the same quads as one device would, and give the same bits)
    if (by_rows && c.pixel_count % (4 * unit) == 0 && c.pixel_count / (4 * unit) >= G) unit *= 4;
    const int units = c.pixel_count / unit;
    if (units < G) return invalid("fewer grid rows (or pixels) than devices");
    awpu_hip *g = new (std::nothrow) awpu_hip();
    if (!g) return AWPU_ERR_NOMEM;
    const auto give_up = [&](int rc) {  // with the error that ended it, not what destroying the parts may leave
        const std::string why = awpu_hip_last_error();
        awpu_hip_destroy(g);
        note_error(why);
        return rc;
    };
    g->cfg = c;
    g->cfg.device = c.devices[0];
    // Row groups of four dealt round-robin (device k owns groups k, k + G, ...) where every device gets at least two of them:
    // the sweep's cost per row grows from the centre of the sine-space grid outwards (fewer shared integer delays), and a
    // group's call takes as long as its slowest device; contiguous slabs otherwise.  Either way a quad is four adjacent grid rows.
    const bool interleave = by_rows && unit == 4 * c.grid_columns && units >= 2 * G;
    int begin = 0;
    for (int k = 0; k < G; k++) {
        awpu_hip_cfg pc = c;
        pc.n_devices = 1;
        pc.device = c.devices[k];
        const int n = units / G + (k < units % G ? 1 : 0);  // the first units % G devices take one more
        std::vector<std::pair<int, int>> ranges;
        if (interleave) {
            for (int u = k; u < units; u += G) ranges.emplace_back(u * unit, unit);
        } else {
            ranges.emplace_back(begin * unit, n * unit);
        }
        pc.pixel_begin = c.pixel_begin + (interleave ? 0 : begin * unit);  // (a part's pixels are what `ranges` says; this only has to be a row start)
        pc.pixel_count = n * unit;
        begin += n;
        awpu_hip *part = nullptr;
        int rc = awpu_hip_create(&part, &pc);
        if (rc == AWPU_OK) {  // what the fan-out needs on top of an ordinary engine
            GroupMember &m = part->member;
            m.ranges = ranges;
            const char *what = "group stream/event creation";
            rc = part->copy_stream.ensure(what);
            for (int b = 0; b < 2 && rc == AWPU_OK; b++) {
                rc = part->ev_copied[b].ensure(hipEventDisableTiming, what);
                if (rc == AWPU_OK) rc = m.ev_swept[b].ensure(hipEventDisableTiming, what);
                if (rc == AWPU_OK) rc = m.ev_staged_read[b].ensure(hipEventDisableTiming, what);
            }
            if (rc == AWPU_OK) rc = m.ev_done.ensure(hipEventDisableTiming, what);
            g->group.parts.push_back(part);
        }
        if (rc != AWPU_OK) return give_up(rc);
    }
    // Direct copies between devices[0] and the others need peer access both ways.  Asked for and CHECKED: a pair
    // without it (another PCIe root, IOMMU settings, a container that hides the links) takes the explicit staged path
    // through pinned host memory -- slower, correct, and said so in awpu_hip_last_error_of / awpu_hip_group_peer_status.
    std::string staged_note;
    for (int k = 0; k < G; k++) {
        GroupMember &m = g->group.parts[k]->member;
        if (c.devices[k] == c.devices[0]) {
            m.peer = env().group_copy >= 2 ? kPeerStaged : kPeerSame;
            continue;
        }
        int can_out = 0, can_in = 0;
        hipError_t e_out = hipDeviceCanAccessPeer(&can_out, c.devices[0], c.devices[k]);
        hipError_t e_in = hipDeviceCanAccessPeer(&can_in, c.devices[k], c.devices[0]);
        if (e_out == hipSuccess && e_in == hipSuccess && can_out && can_in) {
            e_out = hipSetDevice(c.devices[0]);
            if (e_out == hipSuccess) e_out = hipDeviceEnablePeerAccess(c.devices[k], 0);
            e_in = hipSetDevice(c.devices[k]);
            if (e_in == hipSuccess) e_in = hipDeviceEnablePeerAccess(c.devices[0], 0);
        }
        const auto enabled = [](hipError_t e) { return e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled; };
        m.peer = can_out && can_in && enabled(e_out) && enabled(e_in) && env().group_copy < 2 ? kPeerDirect : kPeerStaged;
        if (m.peer == kPeerStaged) {
            staged_note += "device " + std::to_string(c.devices[0]) + " <-> " + std::to_string(c.devices[k]) + ": " +
                           (!(can_out && can_in) ? std::string("hipDeviceCanAccessPeer says no")
                                                 : std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(enabled(e_out) ? e_in : e_out)) + "; ";
        }
    }
    (void) hipGetLastError();
    if (!staged_note.empty())
        g->last_error = "device group without peer access (" + staged_note + "): frames and tiles are staged through pinned host memory";
    AWPU_HIP_TRY(hipSetDevice(c.devices[0]));
    const char *what = "group event creation";
    int rc = g->group.ev_fan.ensure(hipEventDisableTiming, what);
    if (rc == AWPU_OK) rc = g->ev_order.ensure(hipEventDisableTiming, what);
    g->last_stream = g->group.parts[0]->stream;
    for (int b = 0; b < 2 && rc == AWPU_OK; b++) rc = g->group.ev_staged[b].ensure(hipEventDisableTiming, what);
    // a staged part's ev_tile_free[] is recorded on the CALLER's stream (devices[0]) and only waited for on the part's own:
    // an event must be recorded on a stream of the device it was created on, so these belong to devices[0], not the part's
    for (awpu_hip *part : g->group.parts)
        for (int b = 0; b < 2 && rc == AWPU_OK; b++) rc = part->member.ev_tile_free[b].ensure(hipEventDisableTiming, what);
    if (rc != AWPU_OK) return give_up(rc);
    *out = g;
    return AWPU_OK;
}

int group_set_delay_table(awpu_hip *g, const int32_t *off, const float *frac) {  // every device gets the rows of its pixel ranges, back to back
    reset_union_window(g);
    return for_each_part(g, [&](awpu_hip *part) {
        const auto &ranges = part->member.ranges;
        const size_t stride = (size_t) g->cfg.lut_stride;
        if (ranges.size() == 1) {
            const size_t first = (size_t) ranges[0].first * stride;
            return awpu_hip_set_delay_table(part, off + first, frac + first);
        }
        std::vector<int32_t> o((size_t) part->cfg.pixel_count * stride);
        std::vector<float> f(o.size());
        size_t done = 0;
        for (const auto &r : ranges) {
            std::memcpy(&o[done * stride], off + (size_t) r.first * stride, (size_t) r.second * stride * sizeof(int32_t));
            std::memcpy(&f[done * stride], frac + (size_t) r.first * stride, (size_t) r.second * stride * sizeof(float));
            done += (size_t) r.second;
        }
        return awpu_hip_set_delay_table(part, o.data(), f.data());
    });
}

int group_set_active_mics(awpu_hip *g, const int32_t *index, int32_t usable) {
    reset_union_window(g);
    return for_each_part(g, [&](awpu_hip *part) { return awpu_hip_set_active_mics(part, index, usable); });
}

int group_set_mic_gains(awpu_hip *g, const float *gains) {
    return for_each_part(g, [&](awpu_hip *part) { return awpu_hip_set_mic_gains(part, gains); });
}

int group_set_fir_table(awpu_hip *g, const float *coeffs) {
    return for_each_part(g, [&](awpu_hip *part) { return awpu_hip_set_fir_table(part, coeffs); });
}

// enter_stream (awpu_hip.cpp) for the group's host forms.  They enqueue on every part's own stream, so behind a device-form call on a
// caller's stream -- whose tile copies still read the parts' d_power there -- every part's stream waits, not only the first's.  (The
// other way round enter_stream itself serves: the caller's stream waits for the first part's, and the fan-out orders the rest.)
int group_enter_host(awpu_hip *g) {
    const hipStream_t own = g->group.parts[0]->stream;
    if (g->last_stream == own) return AWPU_OK;
    AWPU_HIP_TRY(hipSetDevice(g->cfg.devices[0]));
    AWPU_HIP_TRY(hipEventRecord(g->ev_order, g->last_stream));
    for (awpu_hip *part : g->group.parts) AWPU_HIP_TRY(hipStreamWaitEvent(part->stream, g->ev_order, 0));
    g->last_stream = own;
    return AWPU_OK;
}

int group_process(awpu_hip *g, const float *frames, int batch, float *power) {
    const int rc = enqueue_host_parts(g, frames, batch, power);
    return rc != AWPU_OK ? rc : group_wait(g);
}

int group_process_async(awpu_hip *g, const float *frames, int batch, float *power) {
    const int rc = enqueue_host_parts(g, frames, batch, power);
    if (rc != AWPU_OK) {  // parts before the failing one hold copies from `frames` and into `power` in flight, and
        const std::string why = g->last_error;  // the caller is about to hear "failed": finish them before it does
        for (awpu_hip *part : g->group.parts)
            if (hipSetDevice(part->cfg.device) == hipSuccess) {
                if (part->copy_stream) (void) hipStreamSynchronize(part->copy_stream);
                (void) hipStreamSynchronize(part->stream);
            }
        (void) hipGetLastError();
        note_error(why);
    }
    return rc;
}

int group_wait(awpu_hip *g) {
    return for_each_part(g, [&](awpu_hip *part) { return wait_and_time(part, true); });
}

int group_ingest_block(awpu_hip *g, const void *datagrams, int32_t stride_bytes) {  // every device keeps the whole ring (264 KB per block each, over its own PCIe link)
    if (const int erc = group_enter_host(g); erc != AWPU_OK) return erc;
    const int rc = for_each_part(g, [&](awpu_hip *part) {
        AWPU_CTX(part);
        return enqueue_ingest(part, datagrams, stride_bytes);
    });
    if (rc != AWPU_OK) return rc;
    return for_each_part(g, [&](awpu_hip *part) {
        AWPU_HIP_TRY(hipSetDevice(part->cfg.device));
        AWPU_HIP_TRY(hipStreamSynchronize(part->stream));
        return (int) AWPU_OK;
    });
}

int group_process_ring(awpu_hip *g, float *power) {  // every device sweeps its pixels of its own ring's snapshot
    if (const int erc = group_enter_host(g); erc != AWPU_OK) return erc;
    const int rc = for_each_part(g, [&](awpu_hip *part) {
        AWPU_CTX(part);
        int r = check_ready(part, 1);
        if (r != AWPU_OK) return r;
        if (!part->d_ring) return fail(AWPU_ERR_STATE, "no block ingested yet");
        r = ensure_power(part, (size_t) part->cfg.pixel_count);
        if (r == AWPU_OK) r = launch(part, part->d_ring + part->ring_pos, 1, part->d_power, part->stream, kRing, kTimed);  // (a bracket nobody reads: awpu_hip_process_ring)
        return r != AWPU_OK ? r : enqueue_power_to_host(part, 1, power, (size_t) g->cfg.pixel_count);
    });
    return rc != AWPU_OK ? rc : group_wait(g);
}

int group_synchronize(awpu_hip *g) {
    if (const hipStream_t own = g->group.parts[0]->stream; g->last_stream != own) {  // a device-form call's tile copies, on its caller's stream
        AWPU_HIP_TRY(hipSetDevice(g->cfg.devices[0]));
        AWPU_HIP_TRY(hipStreamSynchronize(g->last_stream));
        g->last_stream = own;
    }
    return for_each_part(g, [](awpu_hip *part) {
        AWPU_HIP_TRY(hipSetDevice(part->cfg.device));
        AWPU_HIP_TRY(hipStreamSynchronize(part->copy_stream));
        AWPU_HIP_TRY(hipStreamSynchronize(part->stream));
        return (int) AWPU_OK;
    });
}

int group_peer_status(awpu_hip *g, int32_t *status, int32_t n) {
    const int have = (int) g->group.parts.size();
    if (n < have) return invalid("status array shorter than the device group");
    for (int k = 0; k < have; k++) {
        const PeerPath peer = g->group.parts[k]->member.peer;
        status[k] = peer == kPeerSame ? AWPU_PEER_SAME_DEVICE : peer == kPeerDirect ? AWPU_PEER_DIRECT : AWPU_PEER_HOST_STAGED;
    }
    return have;
}

int group_stats(awpu_hip *g, awpu_hip_stats *out) {
    const auto &parts = g->group.parts;
    awpu_hip_stats st = parts[0]->stats;
    st.group_exchange = g->stats.group_exchange;
    st.group_ranges = (int32_t) parts[0]->member.ranges.size();
    for (size_t k = 1; k < parts.size(); k++) {
        const awpu_hip_stats &p = parts[k]->stats;
        st.launches += p.launches;
        st.last_kernel_ms = std::max(st.last_kernel_ms, p.last_kernel_ms);   // the slabs run side by side
        st.total_kernel_ms = std::max(st.total_kernel_ms, p.total_kernel_ms);
        st.alg_bytes_frame += p.alg_bytes_frame;
        st.alg_flops_frame += p.alg_flops_frame;
        st.tau_max = std::max(st.tau_max, p.tau_max);
        st.window = std::max(st.window, p.window);
    }
    *out = st;
    return AWPU_OK;
}

}  // namespace awpu::host

// ---- awpu_hip_process_device on a group: frames and power in the memory of devices[0], on the caller's stream there.  What
// travels to the other devices:
//   * batches that the parts sweep with a frame-pair shape (takes_packed_pairs): devices[0] runs the sweep's pack pass ONCE
//     (two frames interleaved, filtered: the packed frame pairs of awpu_hip_pack_frames, the exchange format of the
//     one-process-per-GPU path too) and every other device gets that buffer by ONE linear peer copy on its copy stream and
//     sweeps it as it arrives -- no window cut on devices[0], no pack pass anywhere else;
//   * everything else (single frames, FIR8, exact math, gains): the window of every stream that the tables touch, by one 2-D
//     peer copy per device, and every device runs its whole sweep.
// The parts' pixel ranges are swept concurrently; the tiles return by peer copies on the caller's stream, which thereby waits
// for all of it.  Parts without peer access to devices[0] (kPeerStaged) get the same bytes through pinned host memory: ONE
// copy down on the caller's stream for all of them, one copy up per part on its copy stream; their tiles return the same
// way.  Two buffers everywhere, so that call k+1's copies run beside call k's sweeps.
namespace {

// What travels, where it is now: the packed frame pairs (one linear run of floats), or samples [first, first + pitch) of
// every stream of every frame (rows `pitch` floats apart) -- the caller's frames, or their staged window
struct Payload {
    bool packed = false;
    const float *src = nullptr;
    size_t floats = 0;  // packed: all of them
    int first = 0, pitch = 0;
    size_t rows = 0;    // windows: batch * n_streams
};

// the payload -- of a window payload, samples [lo, lo + w) of every row, packed w apart -- to dst
int copy_payload(const Payload &p, int lo, int w, float *dst, hipMemcpyKind kind, hipStream_t s) {
    if (p.packed) {  // ONE linear copy: the packed pairs of the whole batch
        AWPU_HIP_TRY(hipMemcpyAsync(dst, p.src, p.floats * sizeof(float), kind, s));
    } else {
        AWPU_HIP_TRY(hipMemcpy2DAsync(dst, (size_t) w * sizeof(float), p.src + (lo - p.first), (size_t) p.pitch * sizeof(float),
                                      (size_t) w * sizeof(float), p.rows, kind, s));
    }
    return AWPU_OK;
}

// one call's fan-out
struct Fan {
    awpu_hip *g;
    hipStream_t s;  // the caller's stream on devices[0]
    int batch;
    awpu::FastPlan plan{};  // of the packed pairs
    Payload direct;         // on devices[0]
    Payload staged;         // ... and in pinned memory, where a part is staged
    int pb = 0, gb = 0;     // which of the group's packed / stage buffers this call fills
};

// same GPU as devices[0] (and no copy path forced): the part sweeps the caller's frames, or the group's packed buffer, in place
bool in_place(const awpu_hip *g, const awpu_hip *part) { return part->cfg.device == g->cfg.devices[0] && !env().group_copy; }
// (a staged part is never in place: it is on another device, or AWPU_GROUP_FORCE_COPY=2 made it so)
bool staged(const awpu_hip *part) { return part->member.peer == kPeerStaged; }

// Every part of a group stages the same window -- the union of what the parts' own rows touch -- so that ONE packed buffer
// serves them all (the layout's row length and first sample follow the window).  Results do not depend on the window.
int group_union_window(awpu_hip *g, int batch) {
    if (g->group.union_window_done) return AWPU_OK;
    int lo = g->cfg.hist, hi = 0;
    for (awpu_hip *part : g->group.parts) {
        lo = std::min(lo, part->wstart);
        hi = std::max(hi, part->wstart + part->window);
    }
    for (awpu_hip *part : g->group.parts) {
        if (part->wstart == lo && part->wstart + part->window == hi) continue;
        AWPU_CTX(part);
        part->cfg.window_begin = lo;
        part->cfg.window_end = hi;
        part->prepared = false;
        const int rc = check_ready(part, batch);
        if (rc != AWPU_OK) return part_failed(g, part, rc);
    }
    g->group.union_window_done = true;
    return AWPU_OK;
}

// Step 1: what travels, decided once -- packed frame pairs where every part sweeps them (devices[0] packs them here), else
// the caller's frames -- and ev_fan behind it on the caller's stream
int fan_payload(Fan &f, const float *d_frames) {
    awpu_hip *g = f.g;
    Group &grp = g->group;
    const int dev0 = g->cfg.devices[0];
    bool packed = true;
    for (awpu_hip *part : grp.parts) {
        awpu::FastPlan one{};
        packed = packed && takes_packed_pairs(part, f.batch, &one);
        if (packed && f.plan.wr && (one.wr != f.plan.wr || one.usable_pad != f.plan.usable_pad)) packed = false;
        f.plan = one;
    }
    AWPU_HIP_TRY(hipSetDevice(dev0));
    f.direct.packed = packed;
    if (packed) {
        g->stats.group_exchange = AWPU_EXCHANGE_PACKED_PAIRS;
        awpu_hip *p0 = grp.parts[0];
        const size_t cap = packed_floats_of(p0, f.plan, g->cfg.max_batch);
        if (!grp.packed.holds(cap)) {  // its readers: every part's copies and sweeps, and the caller's stream
            std::vector<StreamOn> readers;
            for (awpu_hip *part : grp.parts) readers.insert(readers.end(), {{part->cfg.device, part->copy_stream}, {part->cfg.device, part->stream}});
            readers.push_back({dev0, f.s});
            if (const int rc = grp.packed.replace(cap, dev0, readers); rc != AWPU_OK) return rc;
        }
        f.pb = grp.packed.next();
        if (grp.packed.used[f.pb])  // buffer pb was read two calls ago: by the peers' copies and by the in-place parts' sweeps
            for (awpu_hip *part : grp.parts)
                AWPU_HIP_TRY(hipStreamWaitEvent(f.s, in_place(g, part) ? part->member.ev_swept[f.pb] : part->ev_copied[f.pb], 0));
        if (const int rc = pack_for_sweep(p0, f.plan, d_frames, f.batch, grp.packed[f.pb], f.s); rc != AWPU_OK) return rc;
        grp.packed.used[f.pb] = true;
        f.direct.src = grp.packed[f.pb];
        f.direct.floats = packed_floats_of(p0, f.plan, f.batch);
    } else {
        g->stats.group_exchange = AWPU_EXCHANGE_WINDOWS;
        f.direct.src = d_frames;
        f.direct.pitch = g->cfg.hist;
        f.direct.rows = (size_t) f.batch * g->cfg.n_streams;
    }
    AWPU_HIP_TRY(hipEventRecord(grp.ev_fan, f.s));  // the frames (or their packed pairs) are in place once the caller's stream gets here
    return AWPU_OK;
}

// Step 2, where a part is staged: what the staged parts need goes down to pinned memory once -- the packed buffer, or the
// union of their windows
int fan_stage(Fan &f) {
    awpu_hip *g = f.g;
    Group &grp = g->group;
    f.staged = f.direct;
    size_t need = 0;
    if (f.direct.packed) {
        need = packed_floats_of(grp.parts[0], f.plan, g->cfg.max_batch);
    } else {
        int lo = g->cfg.hist, hi = 0;
        for (awpu_hip *part : grp.parts) {
            if (!staged(part)) continue;
            const bool compact = part->compact_hist > 0;
            lo = std::min(lo, compact ? part->wstart : 0);
            hi = std::max(hi, compact ? part->wstart + part->compact_hist : part->cfg.hist);
        }
        f.staged.first = lo;
        f.staged.pitch = hi - lo;
        need = (size_t) g->cfg.n_streams * f.staged.pitch * g->cfg.max_batch;
    }
    // (round-4 advisor) Only a buffer that is too SMALL is replaced.  A change of payload -- packed pairs one call, raw windows
    // the next: batches alternating with single frames -- keeps the buffers and their turn: every reuse of stage[gb] already
    // waits for the uploads that read it two calls ago (ev_staged_read below), whatever they carried.
    if (!grp.stage.holds(need)) {  // its readers: every part's uploads, and the caller's stream
        const int dev0 = g->cfg.devices[0];
        std::vector<StreamOn> readers;
        for (awpu_hip *part : grp.parts) readers.push_back({part->cfg.device, part->copy_stream});
        readers.push_back({dev0, f.s});
        if (const int rc = grp.stage.replace(need, dev0, readers); rc != AWPU_OK) return rc;
        grp.stage.turn = 0;
        for (awpu_hip *part : grp.parts) part->member.stage_used[0] = part->member.stage_used[1] = false;
    }
    f.gb = grp.stage.next();
    for (awpu_hip *part : grp.parts)  // stage[gb] was read by the staged parts' uploads two calls ago
        if (staged(part) && part->member.stage_used[f.gb]) AWPU_HIP_TRY(hipStreamWaitEvent(f.s, part->member.ev_staged_read[f.gb], 0));
    if (const int rc = copy_payload(f.direct, f.staged.first, f.staged.pitch, grp.stage[f.gb], hipMemcpyDeviceToHost, f.s); rc != AWPU_OK) return rc;
    f.staged.src = grp.stage[f.gb];
    AWPU_HIP_TRY(hipEventRecord(grp.ev_staged[f.gb], f.s));
    return AWPU_OK;
}

// Step 3, per part: receive the payload (unless it is swept in place), sweep, and -- a staged part -- start the tile's way back
int fan_sweep(const Fan &f, awpu_hip *part) {
    awpu_hip *g = f.g;
    Group &grp = g->group;
    GroupMember &m = part->member;
    const bool packed = f.direct.packed;
    AWPU_CTX(part);
    AWPU_HIP_TRY(hipSetDevice(part->cfg.device));
    int r = ensure_power(part, (size_t) part->cfg.pixel_count * f.batch);
    if (r != AWPU_OK) return r;
    if (in_place(g, part)) {
        AWPU_HIP_TRY(hipStreamWaitEvent(part->stream, grp.ev_fan, 0));
        if (packed) {
            r = sweep_packed(part, f.plan, grp.packed[f.pb], grp.packed.cap(), f.batch, part->d_power, part->stream);
            if (r == AWPU_OK) AWPU_HIP_TRY(hipEventRecord(m.ev_swept[f.pb], part->stream));
        } else {
            r = launch(part, f.direct.src, f.batch, part->d_power, part->stream, kFull);
        }
    } else {
        const bool compact = part->compact_hist > 0;
        const int dev_hist = compact ? part->compact_hist : part->cfg.hist;
        const size_t need_window = (size_t) part->cfg.n_streams * dev_hist * part->cfg.max_batch;
        const size_t need_packed = packed ? packed_floats_of(part, f.plan, part->cfg.max_batch) : 0;
        if (const size_t need = std::max(need_window, need_packed); !m.recv.holds(need)) {  // its readers: the part's own two streams
            const StreamOn readers[] = {{part->cfg.device, part->stream}, {part->cfg.device, part->copy_stream}};
            if (r = m.recv.replace(need, part->cfg.device, readers); r != AWPU_OK) return r;
        }
        // the part's own receive buffer follows the buffer it reads from: the group's packed buffer (pb) or, for a staged
        // part, the staging buffer (gb); a window copy out of the caller's frames takes its own turns
        const int b = staged(part) ? f.gb : (packed ? f.pb : m.recv.next());
        if (m.recv.used[b]) AWPU_HIP_TRY(hipStreamWaitEvent(part->copy_stream, m.ev_swept[b], 0));  // buffer b is free again
        const int lo = compact ? part->wstart : 0;
        if (staged(part)) {
            AWPU_HIP_TRY(hipStreamWaitEvent(part->copy_stream, grp.ev_staged[f.gb], 0));
            if (r = copy_payload(f.staged, lo, dev_hist, m.recv[b], hipMemcpyHostToDevice, part->copy_stream); r != AWPU_OK) return r;
            AWPU_HIP_TRY(hipEventRecord(m.ev_staged_read[f.gb], part->copy_stream));
            m.stage_used[f.gb] = true;
        } else {
            AWPU_HIP_TRY(hipStreamWaitEvent(part->copy_stream, grp.ev_fan, 0));
            if (r = copy_payload(f.direct, lo, dev_hist, m.recv[b], hipMemcpyDeviceToDevice, part->copy_stream); r != AWPU_OK) return r;
        }
        m.recv.used[b] = true;
        AWPU_HIP_TRY(hipEventRecord(part->ev_copied[b], part->copy_stream));
        AWPU_HIP_TRY(hipStreamWaitEvent(part->stream, part->ev_copied[b], 0));
        r = packed ? sweep_packed(part, f.plan, m.recv[b], m.recv.cap(), f.batch, part->d_power, part->stream)
                   : launch(part, m.recv[b], f.batch, part->d_power, part->stream, compact ? kCompact : kFull);
        if (r == AWPU_OK) AWPU_HIP_TRY(hipEventRecord(m.ev_swept[b], part->stream));
        if (r == AWPU_OK && staged(part)) {  // the tile's way back starts on the part's own stream: device -> pinned
            if (const size_t tile = (size_t) part->cfg.pixel_count * part->cfg.max_batch; !m.tile.holds(tile)) {  // its reader: the part's stream
                const StreamOn readers[] = {{part->cfg.device, part->stream}};
                if (r = m.tile.replace(tile, part->cfg.device, readers); r != AWPU_OK) return r;
            }
            if (m.tile.used[f.gb]) AWPU_HIP_TRY(hipStreamWaitEvent(part->stream, m.ev_tile_free[f.gb], 0));
            AWPU_HIP_TRY(hipMemcpyAsync(m.tile[f.gb], part->d_power, (size_t) part->cfg.pixel_count * f.batch * sizeof(float),
                                        hipMemcpyDeviceToHost, part->stream));
            m.tile.used[f.gb] = true;
        }
    }
    if (r == AWPU_OK) AWPU_HIP_TRY(hipEventRecord(m.ev_done, part->stream));
    return r;
}

// a part's tile [batch][its pixels, back to back] -> the group's image [batch][pitch floats]: one 2-D copy per pixel range
int tile_to_image(awpu_hip *part, const float *tile, float *image, size_t pitch_floats, int batch, hipMemcpyKind kind, hipStream_t s) {
    const size_t row = (size_t) part->cfg.pixel_count * sizeof(float);
    size_t done = 0;
    for (const auto &r : part->member.ranges) {
        AWPU_HIP_TRY(hipMemcpy2DAsync(image + r.first, pitch_floats * sizeof(float), tile + done, row, (size_t) r.second * sizeof(float),
                                      (size_t) batch, kind, s));
        done += (size_t) r.second;
    }
    return AWPU_OK;
}

}  // namespace

int awpu::host::group_process_device(awpu_hip *g, const float *d_frames, int batch, float *d_power, hipStream_t stream) {
    Group &grp = g->group;
    AWPU_HIP_TRY(hipSetDevice(g->cfg.devices[0]));
    Fan f{g, stream ? stream : (hipStream_t) grp.parts[0]->stream, batch};
    // behind the group's last call: its tile copies read the parts' d_power on that call's stream, its pack pass wrote grp.packed there
    int rc = enter_stream(g, f.s);
    if (rc == AWPU_OK) rc = for_each_part(g, [&](awpu_hip *part) {
        AWPU_CTX(part);
        return check_ready(part, batch);  // (tables packed: every part's window is known)
    });
    if (rc == AWPU_OK) rc = group_union_window(g, batch);
    if (rc == AWPU_OK) rc = fan_payload(f, d_frames);
    if (rc == AWPU_OK && std::any_of(grp.parts.begin(), grp.parts.end(), staged)) rc = fan_stage(f);
    if (rc == AWPU_OK) rc = for_each_part(g, [&](awpu_hip *part) { return fan_sweep(f, part); });
    if (rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipSetDevice(g->cfg.devices[0]));
    const size_t pitch = (size_t) g->cfg.pixel_count;
    for (awpu_hip *part : grp.parts) {  // tiles back into the caller's [batch][pixel_count] image, range by range
        GroupMember &m = part->member;
        AWPU_HIP_TRY(hipStreamWaitEvent(f.s, m.ev_done, 0));
        if (staged(part)) {
            rc = tile_to_image(part, m.tile[f.gb], d_power, pitch, batch, hipMemcpyHostToDevice, f.s);
            if (rc == AWPU_OK) AWPU_HIP_TRY(hipEventRecord(m.ev_tile_free[f.gb], f.s));
        } else {
            rc = tile_to_image(part, part->d_power, d_power, pitch, batch, hipMemcpyDeviceToDevice, f.s);
        }
        if (rc != AWPU_OK) return rc;
    }
    return AWPU_OK;
}
