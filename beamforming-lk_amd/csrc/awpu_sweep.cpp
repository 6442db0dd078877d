// awpu_sweep.cpp -- the sweep layer of libawpu_hip.so: from a prepared handle and a batch of frames to kernel launches.  In order:
// the diagnostics of the stamped builds, prepare() and the table builders, the small rules every launcher shares (CU count, item
// queues; the XCD pair group is sweep_plan.h's, beside the planners), one launcher per kernel, the dispatch rule (choose_shape
// decides, launch switches) and the packed-frame forms of it.  What awpu_hip.cpp and the runs of blocks call here is declared in
// awpu_handle.h.
#include "awpu_handle.h"

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "cohere_kernels.h"
#include "das_kernels.h"
#include "nd_tile_window.h"
#include "tones_kernels.h"

using namespace awpu::host;

namespace {

// The bracket of a stamped build (AWPU_FAST_DEBUG=16, tuning builds).  Before the launch: `words` of the diagnostics buffer for the
// kernel's stamps, zeroed on the stream where not every slot is written.
int diag_begin(awpu_hip *h, size_t words, bool zero, hipStream_t s, unsigned long long **out) {
    if (const int rc = h->d_diag.ensure(words); rc != AWPU_OK) return rc;  // (one per handle: devices, and launch sizes, differ)
    if (zero) AWPU_HIP_TRY(hipMemsetAsync(h->d_diag, 0, words * sizeof(unsigned long long), s));
    *out = h->d_diag;
    return AWPU_OK;
}

// ... and after it (rc = what finish_launch said; n_waves = 0: no stamps were asked for): the per-wave cycle stamps of the launch
// just enqueued (12 words per wave) to stderr
int diag_end(awpu_hip *h, int rc, size_t n_waves, int wg_waves, const char *tag, hipStream_t s) {
    if (rc != AWPU_OK || n_waves == 0) return rc;
    AWPU_HIP_TRY(hipStreamSynchronize(s));
    std::vector<unsigned long long> hb(n_waves * 12);
    AWPU_HIP_TRY(hipMemcpy(hb.data(), h->d_diag, hb.size() * 8, hipMemcpyDeviceToHost));
    double v[10] = {0};
    std::vector<double> sw(wg_waves, 0), ba(wg_waves, 0);
    for (size_t i = 0; i < n_waves; i++) {
        for (int k = 0; k < 10; k++) v[k] += (double) hb[12 * i + k];
        sw[i % wg_waves] += (double) hb[12 * i + 5];
        ba[i % wg_waves] += (double) hb[12 * i + 8];
    }
    std::fprintf(stderr, "[awpu diag %s] waves %zu, per wave cycles: total %.0f | dma-issue %.0f sweep %.0f (in blocks %.0f = %.1f%%, "
                 "first table wait %.0f) tail %.0f dma-wait %.0f barrier %.0f | per block %.0f\n", tag, n_waves, v[2] / n_waves,
                 v[4] / n_waves, v[5] / n_waves, v[1] / n_waves, 100 * v[1] / v[2], v[0] / n_waves, v[6] / n_waves,
                 v[7] / n_waves, v[8] / n_waves, v[1] / v[3]);
    if (v[9] > 0)  // shader cycles over the 100 MHz real-time counter, both stamped by every wave (MI355X_MICROARCH.md, DVFS give-back item 6)
        std::fprintf(stderr, "[awpu diag %s] in-kernel clock %.3f GHz (cycles %.0f / real time %.2f us per wave)\n", tag, v[2] / v[9] * 0.1,
                     v[2] / n_waves, v[9] / n_waves * 0.01);
    std::fprintf(stderr, "[awpu diag %s] wave slot sweep/barrier kcycles:", tag);
    for (int k = 0; k < wg_waves; k++)
        std::fprintf(stderr, " %d:%.0f/%.0f", k, sw[k] * wg_waves / n_waves / 1e3, ba[k] * wg_waves / n_waves / 1e3);
    std::fprintf(stderr, "\n");
    return AWPU_OK;
}

#ifdef AWPU_TUNING_BUILD
// das_exact_nd_kernel's stamps (8 words per workgroup: where it ran, when, its phases) as a timeline on stderr
int dump_nd_timeline(awpu_hip *h, size_t n_wgs, hipStream_t s) {
    AWPU_HIP_TRY(hipStreamSynchronize(s));
    std::vector<unsigned long long> hb(n_wgs * 8);
    AWPU_HIP_TRY(hipMemcpy(hb.data(), h->d_diag, hb.size() * 8, hipMemcpyDeviceToHost));
    // group by compute unit (XCC, SE, CU of HW_ID), order by start: busy time, gaps between consecutive workgroups
    std::map<unsigned long long, std::vector<std::array<unsigned long long, 5>>> by_cu;
    unsigned long long first = ~0ull, last = 0;
    double ph[3] = {0, 0, 0};
    size_t n = 0;
    for (size_t w = 0; w < n_wgs; w++) {
        const unsigned long long *o = &hb[8 * w];
        if (!o[7]) continue;
        const unsigned hw = (unsigned) o[5], xcc = (unsigned) (o[5] >> 32) & 0xf;
        const unsigned long long cu = ((unsigned long long) xcc << 16) | ((hw >> 8) & 0xff);  // HW_ID: CU_ID [11:8], SH_ID [12], SE_ID [15:13]
        by_cu[cu].push_back({o[0], o[1], o[2], o[3], o[4]});
        first = std::min(first, o[0]);
        last = std::max(last, o[1]);
        for (int k = 0; k < 3; k++) ph[k] += (double) o[2 + k];
        n++;
    }
    double busy = 0, gaps = 0, head = 0, tail = 0;
    size_t n_gaps = 0;
    for (auto &kv : by_cu) {
        auto &v = kv.second;
        std::sort(v.begin(), v.end());
        head += (double) (v.front()[0] - first);
        tail += (double) (last - v.back()[1]);
        for (size_t i = 0; i < v.size(); i++) {
            busy += (double) (v[i][1] - v[i][0]);
            if (i) gaps += (double) v[i][0] - (double) v[i - 1][1], n_gaps++;
        }
    }
    {   // per XCD: when its last workgroup ended (relative to the launch's first stamp), mean busy time of its CUs, and the
        // spread of workgroup durations by position in the item order
        std::map<unsigned, std::array<double, 4>> xs;  // last end, busy sum, CU count, workgroups
        for (auto &kv : by_cu) {
            auto &x = xs[(unsigned) (kv.first >> 16)];
            x[0] = std::max(x[0], (double) (kv.second.back()[1] - first));
            for (auto &w : kv.second) x[1] += (double) (w[1] - w[0]);
            x[2] += 1;
            x[3] += (double) kv.second.size();
        }
        std::fprintf(stderr, "[awpu diag nd] per XCD (last end us / mean busy us / CUs / workgroups):");
        for (auto &kv : xs) std::fprintf(stderr, " %u: %.0f/%.0f/%.0f/%.0f", kv.first, kv.second[0] * 0.01, kv.second[1] / kv.second[2] * 0.01, kv.second[2], kv.second[3]);
        std::vector<double> dur;
        for (size_t w = 0; w < n_wgs; w++) if (hb[8 * w + 7]) dur.push_back((double) (hb[8 * w + 1] - hb[8 * w]) * 0.01);
        std::sort(dur.begin(), dur.end());
        if (!dur.empty()) std::fprintf(stderr, "\n[awpu diag nd] workgroup duration us: min %.1f p10 %.1f median %.1f p90 %.1f max %.1f\n", dur.front(), dur[dur.size() / 10],
                                       dur[dur.size() / 2], dur[dur.size() * 9 / 10], dur.back());
    }
    const double cus = (double) by_cu.size();
    std::fprintf(stderr, "[awpu diag nd] %zu workgroups on %zu CUs, span %.1f us | per CU: busy %.1f us, gaps %.1f us (%.2f us each), idle before first %.1f us, "
                 "after last %.1f us | per workgroup cycles: outside the block %.0f, in the sweep block %.0f, exit %.0f\n", n, by_cu.size(), (double) (last - first) * 0.01,
                 busy / cus * 0.01, gaps / cus * 0.01, n_gaps ? gaps / (double) n_gaps * 0.01 : 0.0, head / cus * 0.01, tail / cus * 0.01, ph[0] / n, ph[1] / n, ph[2] / n);
    return AWPU_OK;
}
#endif

// grow-only device buffer shared by the sweep shapes that pack frames (pairs, quads, FIR8 planes)
int ensure_pack(awpu_hip *h, size_t need) { return ensure_seen_by_live_graphs(h, h->d_pack, need); }

}  // namespace

namespace awpu::host {

// every table prepare() and the launchers build from the delay table and the active-mic list.  (hipFree waits for the device:
// launches still reading the old tables finish first.)
void free_tables(awpu_hip *h) {
    h->d_lut.release();
    h->d_cohere_lut.release();
    h->fast_luts.clear();
    h->d_exact_pair_lut.release();
    for (QuadTable &q : h->quad_tables) q.d.release();
    h->d_nd_starts.release();
    h->d_fir_plane_lut.release();
}

// Pack the reference-format tables into the kernels' layout once both the tables and the
// active-mic list are known.  Validates that no entry reads outside the frame history:
// delay() reads signal[0..256] from &signals[s][offset] (delay.cpp:19-22).
int prepare(awpu_hip *h) {
    const auto &c = h->cfg;
    const int U = h->usable();
    const int P = c.pixel_count;
    int lo = c.hist, hi = -1;
    for (int p = 0; p < P; p++) {
        const int32_t *row = &h->off[(size_t) p * c.lut_stride];
        for (int s = 0; s < U; s++) {
            const int o = row[h->index[s]];
            lo = std::min(lo, o);
            hi = std::max(hi, o);
        }
    }
    const int reach = c.interp == AWPU_INTERP_FIR8 ? awpu::kSamples + 6 : awpu::kSamples;  // last sample read past off
    if (lo < 0 || hi + reach > c.hist - 1) {
        return fail(AWPU_ERR_RANGE, "delay table entry reads outside the frame history");
    }
    if (c.window_end > c.window_begin) {  // a wider window asked for (ranks that exchange packed frames stage the union)
        lo = std::min(lo, c.window_begin);
        hi = std::max(hi, c.window_end - reach - 1);
    }
    h->wstart = lo;
    h->window = hi - lo + reach + 1;
    h->tau_max = awpu::kSamples - lo;

    free_tables(h);
    h->d_index.release();
    h->identity_mics = true;  // the active-mic list is 0 .. usable-1 (awpu_hip_set_active_mics(NULL)): rows need no look-up
    for (int k = 0; k < U && h->identity_mics; k++) h->identity_mics = h->index[k] == k;
    if (const int rc = h->d_index.grow((size_t) U); rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipMemcpy(h->d_index, h->index.data(), (size_t) U * sizeof(int32_t),
                           hipMemcpyHostToDevice));
    h->d_gain.release();
    if (!h->gain.empty()) {
        std::vector<float> compact(U);
        for (int s = 0; s < U; s++) compact[s] = h->gain[h->index[s]];
        if (const int rc = h->d_gain.grow((size_t) U); rc != AWPU_OK) return rc;
        AWPU_HIP_TRY(hipMemcpy(h->d_gain, compact.data(), (size_t) U * sizeof(float), hipMemcpyHostToDevice));
    }
    {   // float offset, inside one frame, of staged row 2*s+q (copy q of active mic s)
        h->d_row_off.release();
        const int upad = (U + 3) & ~3;
        std::vector<int32_t> ro((size_t) 2 * upad + 8, h->index[0] * c.hist + lo);
        for (int s = 0; s < U; s++)
            for (int q = 0; q < 2; q++) ro[2 * s + q] = h->index[s] * c.hist + lo + q;
        if (const int rc = h->d_row_off.grow(ro.size()); rc != AWPU_OK) return rc;
        AWPU_HIP_TRY(hipMemcpy(h->d_row_off, ro.data(), ro.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        // Host-buffer calls upload only the window [lo, lo + compact_hist) of every stream (the rest
        // of the 1024-sample snapshot is never read: SURVEY 8a A10): a third of the PCIe bytes.
        h->d_row_off_compact.release();
        const int ch = ((h->window + 3) & ~3) + 4;
        h->compact_hist = lo + ch <= c.hist ? ch : 0;
        if (c.hist == AWPU_HIST) {  // frames read in place from the ingest ring: rows 2048 floats apart
            std::vector<int32_t> rr(ro.size(), h->index[0] * 2048 + lo);
            for (int s = 0; s < U; s++)
                for (int q = 0; q < 2; q++) rr[2 * s + q] = h->index[s] * 2048 + lo + q;
            if (const int rc = h->d_row_off_ring.grow(rr.size()); rc != AWPU_OK) return rc;
            AWPU_HIP_TRY(hipMemcpy(h->d_row_off_ring, rr.data(), rr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        if (h->compact_hist) {
            for (int s = 0; s < U; s++)
                for (int q = 0; q < 2; q++) ro[2 * s + q] = h->index[s] * h->compact_hist + q;
            for (size_t i = 2 * (size_t) U; i < ro.size(); i++) ro[i] = h->index[0] * h->compact_hist;
            if (const int rc = h->d_row_off_compact.grow(ro.size()); rc != AWPU_OK) return rc;
            AWPU_HIP_TRY(hipMemcpy(h->d_row_off_compact, ro.data(), ro.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
    }

    h->exact_pairs_ok = c.math == AWPU_MATH_F32_EXACT && c.interp == AWPU_INTERP_LERP && awpu::pair_plan(h->window, U, &h->exact_plan);
    h->quad_tables[kQuadExact].plan = h->exact_plan;  // (the quad kernel on raw sample pairs sweeps the pair table's image: one plan)
    // (whole rows here; build_quad_lut(kQuadExactNd) plans again with the tile window once it has walked the table: wr and usable_pad,
    // all that is read before it, do not depend on the window)
    h->exact_nd_ok = h->exact_pairs_ok && awpu::exact_nd_plan(h->window, U, 0, &h->quad_tables[kQuadExactNd].plan);
    h->exact_ndh_ok = h->exact_pairs_ok && awpu::exact_ndh_plan(h->window, U, false, &h->quad_tables[kQuadExactNdh].plan);
    // (AWPU_MATH_F32_FAST sweeps single frames on small grids with the reference-order pixel-per-wave kernel too -- launch() -- : the
    // same plan, the same table)
    h->fast_ndp_ok = c.math == AWPU_MATH_F32_FAST && c.interp == AWPU_INTERP_LERP && awpu::exact_ndh_plan(h->window, U, false, &h->quad_tables[kQuadExactNdh].plan);
    h->exact_ndhs_ok = h->exact_pairs_ok && awpu::exact_ndh_plan(h->window, U, true, &h->quad_tables[kQuadExactNdhStationary].plan);
    // FIR8 with fast math on the four-plane frame-pair layout (das_fir8_plane_kernel)
    h->fir_planes_ok = c.math == AWPU_MATH_F32_FAST && c.interp == AWPU_INTERP_FIR8 && awpu::fir8_plane_plan(h->window, U, &h->fir_plane_plan);
    if (c.math != AWPU_MATH_F32_FAST || c.interp == AWPU_INTERP_FIR8) {
        int chunk = 0;
        if (awpu::das_exact_lds_bytes(h->window, U, &chunk) == 0)
            return invalid("delay window does not fit the LDS budget");
        std::vector<awpu::LutEntry> packed((size_t) P * U);
        for (int p = 0; p < P; p++) {
            const int32_t *orow = &h->off[(size_t) p * c.lut_stride];
            const float *frow = &h->frac[(size_t) p * c.lut_stride];
            awpu::LutEntry *dst = &packed[(size_t) p * U];
            for (int s = 0; s < U; s++) {
                const int id = h->index[s];
                dst[s].off_rel = orow[id] - lo;
                dst[s].frac = frow[id];
                if (c.interp == AWPU_INTERP_FIR8) {  // delay.cpp:32-33: the coefficient row
                    const float get_filter = frow[id] * 100.0f + 0.5f;
                    const int32_t k = (int32_t) get_filter;
                    std::memcpy(&dst[s].frac, &k, sizeof(k));
                }
            }
        }
        if (const int rc = h->d_lut.grow(packed.size()); rc != AWPU_OK) return rc;
        AWPU_HIP_TRY(hipMemcpy(h->d_lut, packed.data(), packed.size() * sizeof(awpu::LutEntry),
                               hipMemcpyHostToDevice));
    } else {
        awpu::FastPlan plan;
        if (!awpu::fast_plan(h->window, U, 1, awpu::kFastLdsBytes, &plan))
            return invalid("delay window does not fit the LDS budget");
    }

    // Pairing of pixels inside a wave of the frame-pair sweep: the shared-read block saves a mic's LDS reads
    // when the two pixels' integer delays coincide.  With the grid's row length known, compare consecutive
    // pixels against vertically adjacent ones on a sample of the table and take the better.
    h->pair_cols = 0;
    {
        const int cols = c.grid_columns;
        if (cols > 0 && P % cols == 0 && c.pixel_begin % cols == 0 && P / cols >= 2) {
            long same_h = 0, same_v = 0, seen = 0;
            const int step = std::max(1, (P - cols) / 4096);
            for (int p = 0; p + cols < P; p += step) {
                if ((p % cols) + 1 >= cols) continue;
                const int32_t *o0 = &h->off[(size_t) p * c.lut_stride];
                const int32_t *oh = &h->off[(size_t) (p + 1) * c.lut_stride];
                const int32_t *ov = &h->off[(size_t) (p + cols) * c.lut_stride];
                for (int s = 0; s < U; s++) {
                    const int id = h->index[s];
                    same_h += o0[id] == oh[id];
                    same_v += o0[id] == ov[id];
                    seen++;
                }
            }
            if (seen > 0 && same_v > same_h) h->pair_cols = cols;
            if (env().pair_cols >= 0) h->pair_cols = env().pair_cols ? cols : 0;  // AWPU_SHAPE=pair_vertical / pair_horizontal: tests force either
        }
    }

    // The quad shape (das_quad_kernel) shares arithmetic between four vertically adjacent pixels wherever their
    // integer delays coincide with the second pixel's: 20 packed VALU instructions per quad and mic, +8 for every
    // pixel that differs (-4 where the third and fourth differ together), against 32 without sharing.  Count it on a sample of the table; take the shape when it
    // saves VALU work at all once its own address adds are counted (measured: a count of 30.2 -- BASELINE c2 -- is
    // 4 % faster than the pair shape, 29.4 -- c3 -- 8 %, 25.3 -- the headline -- 20 %; AWPU_FAST_QUADS=0/1 forces either).
    h->quad_ok = false;
    h->quadh_fits = false;
    h->quadhs_fits = false;
    h->quad_cost = 0.0;
    {
        const int cols = c.grid_columns;
        h->quad_differ = 3.0;
        if (c.interp == AWPU_INTERP_LERP && cols > 0 && P % cols == 0 && c.pixel_begin % cols == 0) {
            const int rows = P / cols;
            long differ = 0, together = 0, seen = 0;  // `together`: pixels 2 and 3 away from the reference as one (4 less)
            const int n_quads = ((rows + 3) / 4) * cols;
            const int step = std::max(1, n_quads / 2048);
            for (int q = 0; q < n_quads; q += step) {
                const int r0 = (q / cols) * 4, col = q % cols;
                const int32_t *o[4];
                for (int k = 0; k < 4; k++) o[k] = &h->off[((size_t) std::min(r0 + k, rows - 1) * cols + col) * c.lut_stride];
                for (int s = 0; s < U; s++) {
                    const int id = h->index[s];
                    differ += (o[0][id] != o[1][id]) + (o[2][id] != o[1][id]) + (o[3][id] != o[1][id]);
                    together += o[2][id] != o[1][id] && o[2][id] == o[3][id];
                }
                seen += U;
            }
            h->quad_cost = seen ? 20.0 + (8.0 * (double) differ - 4.0 * (double) together) / (double) seen : 32.0;
            h->quad_differ = seen ? (double) differ / (double) seen : 3.0;  // pixels of a quad (of three) that leave the reference pixel's address, per mic
            const bool fast = c.math == AWPU_MATH_F32_FAST;
            h->quad_ok = fast && h->quad_cost < 31.0 && awpu::pair_plan(h->window, U, &h->quad_tables[kQuadPairs].plan);
            if (fast && env().quads >= 0) h->quad_ok = env().quads != 0 && awpu::pair_plan(h->window, U, &h->quad_tables[kQuadPairs].plan);
            // the halves layout: a row holds the window less 128 samples, as (sample, sample + 128) pairs (its pack pass applies the gains)
            h->quadh_fits = h->quad_ok && awpu::pair_plan(h->window - 128, U, &h->quad_tables[kQuadHalves].plan);
            h->quadhs_fits = h->quadh_fits && awpu::quadh_stationary_plan(h->window, U, &h->quad_tables[kQuadHalvesStationary].plan);
        }
    }

    auto &st = h->stats;
    st.tau_max = h->tau_max;
    st.window = h->window;
    st.usable = U;
    st.alg_bytes_frame = 4ull * U * h->window + 8ull * P * U + 4ull * P;
    st.alg_flops_frame = 4ull * P * U * awpu::kSamples + 6ull * P * (awpu::kSamples - 2);
    st.kernel_variant = AWPU_KERNEL_NONE;
    h->prepared = true;
    h->table_gen++;  // graphs of awpu_hip_live_block captured against the old tables are stale
    retire_live_graphs(h);
    return AWPU_OK;
}

}  // namespace awpu::host

namespace {

// The fast kernel's table for `fpi` frames per item: per (pixel, active mic s) the weights and
// the LDS byte address of X[off] inside the staged image (das_fast.hip), rows padded to whole
// groups of four with null entries (zero weights, address of a staged row).
int build_fast_lut(awpu_hip *h, awpu::PackLayout layout, int fpi, int image_bytes, const awpu_hip::FastLut **out) {
    for (const auto &l : h->fast_luts)
        if (l.plan.layout == layout && l.plan.fpi == fpi && l.plan.image_bytes == image_bytes) {
            *out = &l;
            return AWPU_OK;
        }
    const auto &c = h->cfg;
    const int U = h->usable(), P = c.pixel_count;
    awpu_hip::FastLut lut;
    const bool pairs = layout != awpu::PackLayout::kSingle;  // frame-pair layout: one image row per mic, 8-byte elements
    const bool planned = layout == awpu::PackLayout::kPairsStationary ? awpu::pair_plan_stationary(h->window, U, &lut.plan)  // every mic resident
                         : pairs                                        ? awpu::pair_plan(h->window, U, &lut.plan)
                                                                        : awpu::fast_plan(h->window, U, fpi, image_bytes, &lut.plan);
    if (!planned) return invalid("delay window does not fit the LDS budget");
    const awpu::FastPlan &plan = lut.plan;
    // rows for whole pixel tiles (the kernels sweep every pixel slot of a workgroup; slots past the
    // grid get null rows) + spare groups: the kernels prefetch entries past the row they sweep
    // (with vertical pixel pairs the partner of a pixel in the last row lies one grid row past the table)
    const int P_pad = (P + (pairs ? h->pair_cols : 0) + 127) / 128 * 128;
    const size_t n = (size_t) P_pad * plan.usable_pad + 4 * awpu::kPairTablePrefetch;
    std::vector<awpu::FastEntry> packed(n, awpu::FastEntry{0.0f, 0u, 0.0f, 0u});
    for (int p = 0; p < P; p++) {
        const int32_t *orow = &h->off[(size_t) p * c.lut_stride];
        const float *frow = &h->frac[(size_t) p * c.lut_stride];
        awpu::FastEntry *dst = &packed[(size_t) p * plan.usable_pad];
        for (int s = 0; s < U; s++) {
            const int id = h->index[s];
            const int off_rel = orow[id] - h->wstart;
            const int q = off_rel & 1;
            const int j = s % plan.chunk;  // mic slot inside its chunk
            dst[s].f = frow[id];
            dst[s].g = 1.0f - frow[id];
            if (!h->gain.empty()) {  // the per-mic gain rides on the two weights
                dst[s].f *= h->gain[id];
                dst[s].g *= h->gain[id];
            }
            dst[s].addr = pairs ? (uint32_t) (j * plan.row_bytes + off_rel * 8)
                                : (uint32_t) ((j * 2 + q) * plan.row_bytes + (off_rel - q) * 4);
        }
    }
    if (const int rc = lut.d.grow(n); rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipMemcpy(lut.d, packed.data(), n * sizeof(awpu::FastEntry), hipMemcpyHostToDevice));
    lut.entries = n;
    h->fast_luts.reserve(8);
    h->fast_luts.push_back(std::move(lut));
    *out = &h->fast_luts.back();
    return AWPU_OK;
}

// The quad shape's table (das_fast.hip, das_quad_kernel): [quad][group of 4 mics][pixel 0..3][mic 0..3] x (f, LDS
// address), quads = groups of four grid rows x columns padded to whole 16-column tiles.  Pixels past the grid
// carry weight 0 and the address of the nearest pixel inside it (they then follow the shared path and add
// nothing); padding mics (usable rounded up to 4) carry weight 0 and the address of their own, zero, row.
int build_quad_lut(awpu_hip *h, QuadLayout layout) {
    QuadTable &table = h->quad_tables[layout];
    if (table.d) return AWPU_OK;
    const auto &c = h->cfg;
    const awpu::FastPlan &plan = table.plan;
    std::vector<uint16_t> starts;  // kQuadExactNd: where each 8-row tile's window begins in a mic's row (nd_tile_window.h); others: none
    if (layout == kQuadExactNd) {
        const int cols = c.grid_columns, wq = plan.wr;
        const int wq_tile = awpu::nd_tile_windows(h->off.data(), c.lut_stride, h->index.data(), h->usable(), plan.usable_pad, c.pixel_count / cols, cols,
                                                  h->wstart, wq, &starts);
        if (!awpu::exact_nd_plan(h->window, h->usable(), wq_tile, &table.plan)) return fail(AWPU_ERR_STATE, "the {next, d} image does not hold the tile window");
        std::vector<unsigned> bytes(starts.size() + 16, 0u);  // + what a wave of a short last chunk reads past the last row (and never uses)
        for (size_t i = 0; i < starts.size(); i++) bytes[i] = 16u * starts[i];
        if (const int rc = h->d_nd_starts.grow(bytes.size()); rc != AWPU_OK) return rc;
        AWPU_HIP_TRY(hipMemcpy(h->d_nd_starts, bytes.data(), bytes.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        h->nd_start_entries = bytes.size();
    }
    const bool halves_nd = layout == kQuadExactNdh || layout == kQuadExactNdhStationary;
    const bool raw = layout == kQuadExact || layout == kQuadExactNd || halves_nd;
    const float centre = raw ? 0.0f : 0.5f;  // the reference-order sweeps take the fraction as it is (mimo.cpp:126)
    const int elem = layout == kQuadExactNd || halves_nd ? 16 : 8;  // bytes per LDS element: {next, d} of a frame pair / of the two halves, or one sample pair
    const int U = h->usable(), cols = c.grid_columns, rows = c.pixel_count / cols;
    const int groups = plan.usable_pad / 4;
    // (the {next, d} kernel gives a wave two quads, one quad row apart: its table has an even number of quad rows, the last one clamped;
    // ... the single-frame form two quads one COLUMN apart: its table has whole tiles of 32 columns)
    const int cols_pad = halves_nd ? (cols + 31) / 32 * 32 : (cols + 15) / 16 * 16, rows4 = layout == kQuadExactNd ? ((rows + 3) / 4 + 1) / 2 * 2 : (rows + 3) / 4;
    const size_t n = (size_t) rows4 * cols_pad * groups * 16 + 2 * awpu::kQuadTablePrefetch;  // spare groups: the sweep prefetches one past the end
    std::vector<awpu::QuadEntry> packed(n, awpu::QuadEntry{0.0f, 0u});
    for (int r4 = 0; r4 < rows4; r4++)
        for (int col = 0; col < cols_pad; col++) {
            awpu::QuadEntry *dst = &packed[((size_t) r4 * cols_pad + col) * groups * 16];
            for (int q = 0; q < 4; q++) {
                const int row = 4 * r4 + q;
                const bool inside = row < rows && col < cols;
                const size_t p = (size_t) std::min(row, rows - 1) * cols + std::min(col, cols - 1);
                const int32_t *orow = &h->off[p * c.lut_stride];
                const float *frow = &h->frac[p * c.lut_stride];
                for (int s = 0; s < plan.usable_pad; s++) {
                    awpu::QuadEntry &e = dst[((s >> 2) * 4 + q) * 4 + (s & 3)];
                    const int j = s % plan.chunk;  // mic slot inside its chunk
                    if (s < U) {
                        const int id = h->index[s];
                        int off_rel = orow[id] - h->wstart;
                        if (layout == kQuadExactNd)  // the LDS row begins at the tile's start
                            off_rel -= starts[((size_t) (r4 / 2) * (cols_pad / 16) + col / 16) * plan.usable_pad + s];
                        e.f = inside ? frow[id] - centre : 0.0f;  // centred weight (das_fast.hip, das_quad_kernel); exact: as it is
                        e.addr = (uint32_t) (j * plan.row_bytes + off_rel * elem);
                    } else {  // padding mic: silence (the pack passes write zero rows)
                        e.f = 0.0f;
                        e.addr = (uint32_t) (j * plan.row_bytes);
                    }
                }
            }
        }
    if (const int rc = table.d.grow(n); rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipMemcpy(table.d, packed.data(), n * sizeof(awpu::QuadEntry), hipMemcpyHostToDevice));
    table.entries = n;
    return AWPU_OK;
}

// The reference-order sweep on the frame-pair layout (das_exact_pair_kernel): the table is the pair shape's with the
// UNSCALED fraction in .f (gains go on the samples, as in das_exact_kernel) and padding entries -- mics usable ..
// usable_pad-1, and whole rows past the grid -- that read a row of zeros with fraction 0 (they add +0).
int build_exact_pair_lut(awpu_hip *h) {
    if (h->d_exact_pair_lut) return AWPU_OK;
    const auto &c = h->cfg;
    const awpu::FastPlan &plan = h->exact_plan;
    const int U = h->usable(), P = c.pixel_count;
    const int P_pad = (P + h->pair_cols + 127) / 128 * 128;  // whole tiles; with vertical pairs the partner of a last-row pixel lies one grid row past the table
    const size_t n = (size_t) P_pad * plan.usable_pad + 4 * awpu::kPairTablePrefetch;  // spare groups: the block prefetches one past a row's end
    std::vector<awpu::FastEntry> packed(n);
    for (size_t i = 0; i < n; i++)  // null entry of slot s: the zero row of its own slot in the last chunk, or any row with fraction 0 ...
        packed[i] = awpu::FastEntry{0.0f, (uint32_t) ((int) (i % plan.usable_pad) % plan.chunk * plan.row_bytes), 0.0f, 0u};
    for (int p = 0; p < P; p++) {
        const int32_t *orow = &h->off[(size_t) p * c.lut_stride];
        const float *frow = &h->frac[(size_t) p * c.lut_stride];
        awpu::FastEntry *dst = &packed[(size_t) p * plan.usable_pad];
        for (int s = 0; s < U; s++) {
            const int id = h->index[s];
            dst[s].f = frow[id];  // the reference's `fraction`, mimo.cpp:126
            dst[s].addr = (uint32_t) ((s % plan.chunk) * plan.row_bytes + (orow[id] - h->wstart) * 8);
        }
    }
    if (const int rc = h->d_exact_pair_lut.grow(n); rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipMemcpy(h->d_exact_pair_lut, packed.data(), n * sizeof(awpu::FastEntry), hipMemcpyHostToDevice));
    h->exact_pair_lut_entries = n;
    return AWPU_OK;
}

// FIR8 on the four-plane layout (das_fir8_plane_kernel): one dword per (pixel, mic) -- address, plane, coefficient row --; four
// spare: the block requests entries four items ahead.  Null entries (the padding of a row, the spares) read row 0 with the zero
// coefficient row.
int build_fir8_plane_lut(awpu_hip *h) {
    if (h->d_fir_plane_lut) return AWPU_OK;
    const awpu::FastPlan &pp = h->fir_plane_plan;
    const int U = h->usable(), P = h->cfg.pixel_count;
    const int row_entries = pp.usable_pad;  // (a multiple of 4, like the chunk: the block sweeps groups of four items)
    const uint32_t plane_bytes = (uint32_t) pp.row_bytes / 4;
    std::vector<uint32_t> packed((size_t) P * row_entries + awpu::kFir8PlaneTablePrefetch, awpu::fir8_plane_word(0, 0, awpu::kFir8ZeroRow));
    for (int p = 0; p < P; p++) {
        const int32_t *orow = &h->off[(size_t) p * h->cfg.lut_stride];
        const float *frow = &h->frac[(size_t) p * h->cfg.lut_stride];
        for (int m = 0; m < U; m++) {
            const int id = h->index[m];
            const int32_t k = (int32_t) (frow[id] * 100.0f + 0.5f);  // delay.cpp:32-33: the coefficient row
            const uint32_t first = (uint32_t) (orow[id] - h->wstart);  // row element of X[off]
            const uint32_t addr = (uint32_t) (m % pp.chunk) * pp.row_bytes + (first & 3) * plane_bytes + (first >> 2) * 8;
            packed[(size_t) p * row_entries + m] = awpu::fir8_plane_word(addr, first & 3, (uint32_t) k);
        }
    }
    if (const int rc = h->d_fir_plane_lut.grow(packed.size()); rc != AWPU_OK) return rc;
    AWPU_HIP_TRY(hipMemcpy(h->d_fir_plane_lut, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    h->fir_plane_lut_entries = packed.size();
    return AWPU_OK;
}

// Kernel shape for a call.  AWPU_FAST_VARIANT="fpi,ppw[,nw]" overrides the heuristic (tuning
// knob, read once): fpi frames per item, ppw pixels per wave, nw = 8 (8-wave workgroups, two per
// CU) or 32 (the double-buffered 16-wave shape, one per CU).
void choose_fast_variant(awpu_hip *h, int batch, int *fpi, int *ppw, int *nw) {
    const int env_fpi = env().fpi, env_ppw = env().ppw, env_nw = env().nw;
    // Prefer the double-buffered shape with the most pixels per wave that still gives every CU
    // a workgroup; small grids fall back to 8-wave workgroups with fewer pixels per wave.
    const long P = h->cfg.pixel_count;
    auto wgs = [&](long pix_per_wg) { return (P + pix_per_wg - 1) / pix_per_wg * batch; };
    *fpi = 1;
    if (wgs(128) >= 256) {
        *nw = 32;
        *ppw = 8;
    } else if (wgs(64) >= 256) {
        *nw = 32;
        *ppw = 4;
    } else {
        *nw = 8;
        *ppw = wgs(32) >= 512 ? 4 : 2;
    }
    if (env_fpi == 1 || env_fpi == 2) *fpi = env_fpi;
    if (env_ppw == 2 || env_ppw == 4 || env_ppw == 8) *ppw = env_ppw;
    if (env_nw == 8 || env_nw == 32 || env_nw == 24) *nw = env_nw;
    if (*nw == 32) {
        *fpi = 1;
        if (*ppw < 4) *ppw = 4;
    }
    if (*nw == 24) {
        *fpi = 1;
        *ppw = 4;
    }
    if (*fpi == 2 && *ppw == 8) *ppw = 4;
    if (*fpi == 2 && batch < 2) *fpi = 1;
}

// a launch is over: close the timing bracket and count it (also on the diagnostic paths)
int finish_launch(awpu_hip *h, int batch, hipStream_t s, bool timed, int kernel_id) {
    h->stats.kernel_variant = kernel_id;
    if (timed) AWPU_HIP_TRY(hipEventRecord(h->ev_end, s));
    h->stats.launches += 1;
    h->stats.frames += (uint64_t) batch;
    return AWPU_OK;
}

// compute units of the handle's device (asked once)
int cu_count(awpu_hip *h) {
    if (h->n_cus < 1 && (hipDeviceGetAttribute(&h->n_cus, hipDeviceAttributeMultiprocessorCount, h->cfg.device) != hipSuccess || h->n_cus < 1))
        h->n_cus = 256;
    return h->n_cus;
}

// Persistent workgroups (one per CU) that take their `items` from queues, one per XCD: an eighth of every XCD's run goes to the
// queue common to the chip (the XCDs' speeds differ by ~6 %); short runs: one queue for the chip.
int arm_item_queues(awpu_hip *h, int items, unsigned **queue, int32_t *wgs, int32_t *tail) {
    if (const int rc = h->d_nd_queue.ensure(9); rc != AWPU_OK) return rc;
    *queue = h->d_nd_queue;
    *wgs = cu_count(h);
    const int per = (items + 7) / 8;
    *tail = per >= 32 ? (per + 7) / 8 : per;
    return AWPU_OK;
}

// floats of the pack buffer for the frame pairs of `frames` frames: `rows` rows per pair of `wr` elements of `floats` floats
size_t pair_pack_floats(int frames, int rows, int wr, int floats) { return (size_t) ((frames + 1) / 2) * rows * wr * floats; }

// The six fields every sweep kernel's arguments share -- power, usable, usable_pad, pixel_count, chunk, batch -- (das_kernels.h keeps
// one struct per kernel); a launcher sets every other field of its struct itself
template <class Args>
void fill_shared(Args &a, const awpu_hip *h, const awpu::FastPlan &plan, int batch, float *d_power) {
    a.power = d_power;
    a.usable = h->usable();
    a.usable_pad = plan.usable_pad;
    a.pixel_count = h->cfg.pixel_count;
    a.chunk = plan.chunk;
    a.batch = batch;
}

int launch_exact_pairs(awpu_hip *h, const SweepCall &call) {
    if (const int rc = build_exact_pair_lut(h); rc != AWPU_OK) return rc;
    const awpu::FastPlan &pp = h->exact_plan;
    if (const int prc = ensure_pack(h, pair_pack_floats(std::max(h->cfg.max_batch, call.batch), pp.usable_pad, pp.wr, 2)); prc != AWPU_OK) return prc;
    awpu::ExactPairArgs a{};
    fill_shared(a, h, pp, call.batch, call.power);
    a.packed = h->d_pack;
    a.lut = h->d_exact_pair_lut;
    a.sums = call.opts.sums;
    a.wp = pp.wr;
    a.cols = h->pair_cols;
    a.tiles = awpu::pair_tiles(a.pixel_count, a.cols);
    a.n_pairs = (call.batch + 1) / 2;
    a.pair_group = awpu::xcd_pair_group((size_t) pp.usable_pad * pp.wr * 8, a.n_pairs);
    if (call.opts.timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, call.stream));
    AWPU_HIP_TRY(awpu::launch_pack_pairs(call.frames, h->cfg.n_streams, call.hist_eff, call.wstart_eff, h->d_index, h->usable(), pp.usable_pad,
                                         h->d_gain, pp.wr, call.batch, h->d_pack, false, call.stream));  // raw samples: no stencil in front of the reference's order
    AWPU_HIP_TRY(awpu::launch_das_exact_pairs(a, {h->exact_pair_lut_entries, h->d_pack.cap}, call.stream));
    return finish_launch(h, call.batch, call.stream, call.opts.timed, AWPU_KERNEL_EXACT_PAIR);
}

// ... four vertically adjacent pixels per wave where the row length is known (das_exact_quad_kernel): same bits, fewer LDS reads
int launch_exact_quads(awpu_hip *h, const SweepCall &call) {
    if (const int rc = build_quad_lut(h, kQuadExact); rc != AWPU_OK) return rc;
    const QuadTable &table = h->quad_tables[kQuadExact];
    const awpu::FastPlan &pp = table.plan;
    if (const int prc = ensure_pack(h, pair_pack_floats(std::max(h->cfg.max_batch, call.batch), pp.usable_pad, pp.wr, 2)); prc != AWPU_OK) return prc;
    awpu::ExactQuadArgs a{};
    fill_shared(a, h, pp, call.batch, call.power);
    a.packed = h->d_pack;
    a.lut = table.d;
    a.sums = call.opts.sums;
    a.wp = pp.wr;
    a.cols = h->cfg.grid_columns;
    a.rows = h->cfg.pixel_count / a.cols;
    a.tiles = awpu::quad_tiles(a.rows, a.cols);
    a.n_pairs = (call.batch + 1) / 2;
    a.pair_group = awpu::xcd_pair_group((size_t) pp.usable_pad * pp.wr * 8, a.n_pairs);
    if (call.opts.timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, call.stream));
    AWPU_HIP_TRY(awpu::launch_pack_pairs(call.frames, h->cfg.n_streams, call.hist_eff, call.wstart_eff, h->d_index, h->usable(), pp.usable_pad,
                                         h->d_gain, pp.wr, call.batch, h->d_pack, false, call.stream));
    AWPU_HIP_TRY(awpu::launch_das_exact_quads(a, {table.entries, h->d_pack.cap}, call.stream));
    return finish_launch(h, call.batch, call.stream, call.opts.timed, AWPU_KERNEL_EXACT_QUAD);
}

// ... on the {next, d} layout (das_exact_nd_kernel, round 5): cur - next formed once per sample by the pack pass; nq quads per wave
int launch_exact_nd(awpu_hip *h, const SweepCall &call, int nq, const float *prepacked = nullptr, size_t prepacked_floats = 0) {
    int rc = build_quad_lut(h, kQuadExactNd);
    if (rc != AWPU_OK) return rc;
    const QuadTable &table = h->quad_tables[kQuadExactNd];
    const awpu::FastPlan &pp = table.plan;
    if (!prepacked)
        if (const int prc = ensure_pack(h, pair_pack_floats(std::max(h->cfg.max_batch, call.batch), pp.usable_pad, pp.wr, 4)); prc != AWPU_OK) return prc;
    awpu::ExactNdArgs a{};
    fill_shared(a, h, pp, call.batch, call.power);
    a.packed = prepacked ? prepacked : h->d_pack;
    a.lut = table.d;
    a.sums = call.opts.sums;
    a.wq = pp.wr;
    a.wq_tile = pp.row_bytes / 16;
    a.starts = h->d_nd_starts;
    a.start_entries = h->nd_start_entries;
    a.cols = h->cfg.grid_columns;
    a.rows = h->cfg.pixel_count / a.cols;
    a.nq = nq;
    a.tiles = awpu::nd_tiles(a.rows, a.cols, nq);
    a.n_pairs = (call.batch + 1) / 2;
    a.pair_group = awpu::xcd_pair_group((size_t) pp.usable_pad * pp.wr * 16, a.n_pairs, env().pair_group);
    // Four pairs instead of two where four pairs' rows are at most 6 MiB (the headline: 5.7 MB): every XCD then walks the table twice per
    // launch instead of four times, and a tile stages only its window of a row.  Alternating runs on one box: -0.30 % (5.378 against
    // 5.394 ms per step; profiles/r13_tile_window_rate.txt).  Larger pairs (c3, the c5 slab) keep the rule above: not measured.
    if (env().pair_group <= 0 && a.pair_group == 2 && a.n_pairs >= 4 && (size_t) pp.usable_pad * pp.wr * 16 * 4 <= (6u << 20)) a.pair_group = 4;
    {   // the item list: rebuilt (by the launcher, on the stream) when the batch, the pair group or the tile shape changed
        const size_t items = (size_t) a.n_pairs * a.tiles;
        const long long key = ((long long) a.n_pairs << 24) | ((long long) a.pair_group << 8) | nq;
        if (!h->d_nd_items.holds(items)) {
            retire_live_graphs(h);
            AWPU_HIP_TRY(hipStreamSynchronize(call.stream));  // (a sweep in flight may still read the old list)
            if (rc = h->d_nd_items.grow(items); rc != AWPU_OK) return rc;
            h->nd_items_key = -1;
        }
        a.items = h->d_nd_items;
        a.build_items = h->nd_items_key != key;
        h->nd_items_key = key;
    }
    if (rc = arm_item_queues(h, a.n_pairs * a.tiles, &a.queue, &a.wgs, &a.tail); rc != AWPU_OK) return rc;
#ifdef AWPU_TUNING_BUILD
    if (const char *v = std::getenv("AWPU_ND_TAIL")) {  // percent of a run
        const int per = (a.n_pairs * a.tiles + 7) / 8;
        a.tail = std::max(1, std::atoi(v) >= 100 ? per : per * std::atoi(v) / 100);
    }
#endif
    if (call.opts.timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, call.stream));
    if (!prepacked) {  // (the pack pass zeroes the sweep's queues too: one dispatch less than a memset between the two)
        AWPU_HIP_TRY(awpu::launch_pack_nd(call.frames, h->cfg.n_streams, call.hist_eff, call.wstart_eff, h->d_index, h->usable(), pp.usable_pad, h->d_gain,
                                          pp.wr, call.batch, h->d_pack, a.queue, call.stream));
        a.queue_zeroed = 1;
    }
#ifdef AWPU_TUNING_BUILD
    const size_t n_wgs = std::min<size_t>((size_t) a.n_pairs * a.tiles, (size_t) a.wgs);
    if (env().debug & 16)  // per-workgroup timeline (where, when, phases)
        if (const int drc = diag_begin(h, n_wgs * 8, true, call.stream, &a.debug_out); drc != AWPU_OK) return drc;
#endif
    AWPU_HIP_TRY(awpu::launch_das_exact_nd(a, {table.entries, prepacked ? prepacked_floats : h->d_pack.cap}, call.stream));
    rc = finish_launch(h, call.batch, call.stream, call.opts.timed, AWPU_KERNEL_EXACT_ND);
#ifdef AWPU_TUNING_BUILD
    if (rc == AWPU_OK && (env().debug & 16)) return dump_nd_timeline(h, n_wgs, call.stream);
#endif
    return rc;
}

// Does launch() sweep a batch of AWPU_MATH_F32_EXACT with das_exact_nd_kernel, and with how many quads per wave?  (The rule of launch()
// and of the packed-frame entry points: asked before anything is packed.)
bool takes_exact_nd(awpu_hip *h, int batch, int *nq) {
    if (!h->exact_pairs_ok || !h->exact_nd_ok || h->cfg.grid_columns < 1) return false;
    const ExactShape ex = env().exact_pairs;
    if (ex == ExactShape::kVerify || ex == ExactShape::kPair || ex == ExactShape::kQuad) return false;
    const int cols = h->cfg.grid_columns, rows = h->cfg.pixel_count / cols;
    // (quad_differ < 1.5: on average fewer than half of a quad's pixels leave the reference pixel's address for a mic; a square
    // array's vertical and horizontal neighbours coincide equally often -- pair_cols stays 0 there -- and quads still pay)
    const bool quads_pay = h->cfg.pixel_count % cols == 0 && h->cfg.pixel_begin % cols == 0 && h->quad_differ < 1.5;
    if ((!(h->pair_cols > 0 || quads_pay) && !forces_exact_nd(ex)) || rows < 4) return false;  // (a forced shape runs on any table: the random tests)
    // two quads per wave where that still fills the chip (AWPU_SHAPE=exact_nd1 / exact_nd2: one / two everywhere)
    const long wgs2 = (long) awpu::nd_tiles(rows, cols, 2) * ((batch + 1) / 2);
    *nq = ex == ExactShape::kNd1 ? 1 : ex == ExactShape::kNd2 ? 2 : (rows >= 8 && wgs2 >= 512 ? 2 : 1);
    return true;
}

// The completion flag of the synchronous one-frame host call (das_kernels.h: DoneFlag; das_fast.hip: store_tile_and_signal): what the
// next armed launch of `workgroups` workgroups gets, and -- once that launch has gone out -- what the handle remembers and the
// call that asked for the flag (SweepOpts::flag) is told.
int arm_done_flag(awpu_hip *h, unsigned long long workgroups, awpu::DoneFlag *out) {
    if (!h->d_done_counter) {
        if (const int rc = h->d_done_counter.grow(1); rc != AWPU_OK) return rc;
        AWPU_HIP_TRY(hipMemsetAsync(h->d_done_counter, 0, sizeof(unsigned long long), h->stream));
        AWPU_HIP_TRY(hipStreamSynchronize(h->stream));  // (the handle's own stream: nothing device-wide from inside a sweep call)
        if (const int rc = h->h_done_flag.grow(16); rc != AWPU_OK) return rc;  // (a cache line of its own)
        *h->h_done_flag = 0;
        h->done_total = 0;
    }
    out->counter = h->d_done_counter;
    out->flag = h->h_done_flag;
    out->target = h->done_total + workgroups;
    out->seq = h->done_seq + 1;
    return AWPU_OK;
}
void done_flag_armed(awpu_hip *h, const awpu::DoneFlag &d, bool *will_raise) {
    h->done_total = d.target;
    h->done_seq = d.seq;
    *will_raise = true;
}

// single frames in the reference's order: the halves form of the {next, d} layout (das_exact_ndh_kernel) -- every mic resident and
// staged by the workgroups themselves (one array), or chunked behind a pack pre-pass
int launch_exact_ndh(awpu_hip *h, const SweepCall &call, bool stationary, int nq, bool pixel_per_wave = false) {
    const QuadLayout layout = stationary ? kQuadExactNdhStationary : kQuadExactNdh;
    int rc = build_quad_lut(h, layout);
    if (rc != AWPU_OK) return rc;
    const QuadTable &table = h->quad_tables[layout];
    const awpu::FastPlan &pp = table.plan;
    if (!stationary) {
        const size_t need = std::max((size_t) h->cfg.max_batch, (size_t) call.batch) * pp.usable_pad * pp.wr * 4;
        if (const int prc = ensure_pack(h, need); prc != AWPU_OK) return prc;
    }
    awpu::ExactNdhArgs a{};
    fill_shared(a, h, pp, call.batch, call.power);
    a.packed = stationary ? nullptr : h->d_pack;
    a.frames = call.frames;
    a.lut = table.d;
    a.index = h->d_index;
    a.gain = h->d_gain;
    a.sums = call.opts.sums;
    a.n_streams = h->cfg.n_streams;
    a.pitch = call.hist_eff;
    a.wstart = call.wstart_eff;
    a.wh = pp.wr;
    a.cols = h->cfg.grid_columns;
    a.rows = h->cfg.pixel_count / a.cols;
    a.nq = nq;
    a.tiles = pixel_per_wave ? awpu::ndp_tiles(a.rows, a.cols) : awpu::ndh_tiles(a.rows, a.cols, nq);
    a.lut_cols = (a.cols + 31) / 32 * 32;
    a.identity = h->identity_mics;
    if (call.opts.flag && call.stream == h->stream && stationary && nq == 1 && !pixel_per_wave) {  // (the one-frame host call: live_host_call)
        if (rc = arm_done_flag(h, (unsigned long long) call.batch * a.tiles, &a.done); rc != AWPU_OK) return rc;
    }
    if (call.opts.timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, call.stream));
    if (!stationary)
        AWPU_HIP_TRY(awpu::launch_pack_ndh(call.frames, h->cfg.n_streams, call.hist_eff, call.wstart_eff, a.identity ? nullptr : h->d_index, h->usable(), pp.usable_pad, h->d_gain, pp.wr,
                                           call.batch, h->d_pack, call.stream));
    if (pixel_per_wave) {
        AWPU_HIP_TRY(awpu::launch_das_exact_ndp(a, {table.entries, h->d_pack.cap}, call.stream));
    } else {
        AWPU_HIP_TRY(awpu::launch_das_exact_ndh(a, stationary, {table.entries, stationary ? 0 : h->d_pack.cap}, call.stream));
    }
    if (a.done.flag) done_flag_armed(h, a.done, call.opts.flag);  // (the launch went out: its workgroups will count themselves)
    return finish_launch(h, call.batch, call.stream, call.opts.timed, pixel_per_wave ? AWPU_KERNEL_EXACT_NDP : stationary ? AWPU_KERNEL_EXACT_NDH_STATIONARY : AWPU_KERNEL_EXACT_NDH);
}

int launch_exact(awpu_hip *h, const SweepCall &call) {
    awpu::SweepArgs a{};
    a.frames = call.frames;
    a.lut = h->d_lut;
    a.index = h->d_index;
    a.power = call.power;
    a.gain = h->d_gain;
    a.sums = call.opts.sums;  // (choose_shape: EXACT + FIR8 only)
    a.n_streams = h->cfg.n_streams;
    a.hist = call.hist_eff;
    a.usable = h->usable();
    a.pixel_count = h->cfg.pixel_count;
    a.wstart = call.wstart_eff;
    a.window = h->window;
    a.batch = call.batch;
    if (call.opts.timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, call.stream));
    if (h->cfg.interp == AWPU_INTERP_FIR8) {
        // AWPU_MATH_F32_EXACT: the reference's rounding, a multiply and an add per tap; AWPU_MATH_F32_FAST (a launch too small for the
        // plane kernel): one FMA per tap
        AWPU_HIP_TRY(awpu::launch_das_fir8(a, h->d_fir, h->cfg.math == AWPU_MATH_F32_EXACT, call.stream));
    } else {
        AWPU_HIP_TRY(awpu::launch_das_exact(a, h->cfg.math == AWPU_MATH_BF16_ACC, call.stream));
    }
    return finish_launch(h, call.batch, call.stream, call.opts.timed, h->cfg.interp == AWPU_INTERP_FIR8 ? AWPU_KERNEL_FIR8 : AWPU_KERNEL_EXACT_VERIFY);
}

// FIR8 on the four-plane frame-pair layout (das_fir8_plane_kernel): a lane owns four consecutive outputs
int launch_fir8_planes(awpu_hip *h, const SweepCall &call) {
    if (const int rc = build_fir8_plane_lut(h); rc != AWPU_OK) return rc;
    const awpu::FastPlan &pp = h->fir_plane_plan;
    const int U = h->usable(), P = h->cfg.pixel_count, cols = h->cfg.grid_columns;
    if (const int prc = ensure_pack(h, pair_pack_floats(h->cfg.max_batch, U, pp.wr, 2)); prc != AWPU_OK) return prc;
    awpu::PairArgs pa{};
    fill_shared(pa, h, pp, call.batch, call.power);
    pa.packed = h->d_pack;
    pa.wp = pp.wr;
    pa.pair_group = awpu::xcd_pair_group((size_t) U * pp.wr * 8, (call.batch + 1) / 2);
    // vertical pixel quads (samples shared between pixels of one column with the same integer delay) where the grid's row
    // length is known and the rows are staged at the pitch that block is generated for; AWPU_FIR8_SHARE=0: consecutive pixels
    if (env().fir_share != 0 && cols > 0 && P % cols == 0 && h->cfg.pixel_begin % cols == 0 && (uint32_t) pp.wr * 2u == awpu::kFirStaticPlaneBytesHost)
        pa.cols = cols;
    if (call.opts.timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, call.stream));
    AWPU_HIP_TRY(awpu::launch_pack_planes(call.frames, h->cfg.n_streams, call.hist_eff, call.wstart_eff, h->d_index, U, h->d_gain, pp.wr,
                                          call.batch, h->d_pack, call.stream));
    AWPU_HIP_TRY(awpu::launch_das_fir8_planes(pa, h->d_fir_plane_lut, h->d_fir, env().quad_variant, {h->fir_plane_lut_entries, h->d_pack.cap}, call.stream));
    return finish_launch(h, call.batch, call.stream, call.opts.timed, AWPU_KERNEL_FIR8_PLANES);
}

// frame-pair shape: two frames per item, for batches on grids that fill the chip
int launch_pairs(awpu_hip *h, const awpu_hip::FastLut *plut, const SweepCall &call, int stationary_tiles = 0, const float *prepacked = nullptr,
                 size_t prepacked_floats = 0) {
    const awpu::FastPlan &pp = plut->plan;
    // the stationary shape stages its pairs itself, straight from the caller's frames (no pack pre-pass, no packed buffer)
    const bool self_staged = stationary_tiles > 0 && !prepacked;
    if (!prepacked && !self_staged)
        if (const int prc = ensure_pack(h, pair_pack_floats(h->cfg.max_batch, h->usable(), pp.wr, 2)); prc != AWPU_OK) return prc;
    awpu::PairArgs pa{};
    fill_shared(pa, h, pp, call.batch, call.power);
    pa.packed = prepacked ? prepacked : (self_staged ? nullptr : h->d_pack);
    if (self_staged) {
        pa.frames = call.frames;
        pa.index = h->d_index;
        pa.n_streams = h->cfg.n_streams;
        pa.hist = call.hist_eff;
        pa.wstart = call.wstart_eff;
    }
    pa.lut = plut->d;
    pa.wp = pp.wr;
    pa.cols = h->pair_cols;
    pa.tiles = awpu::pair_tiles(h->cfg.pixel_count, h->pair_cols);
    pa.n_pairs = (call.batch + 1) / 2;
    pa.pair_group = awpu::xcd_pair_group((size_t) h->usable() * pp.wr * 8, pa.n_pairs);
    pa.debug = env().debug;
    size_t n_waves = 0;
    if (stationary_tiles > 0) pa.debug &= ~16;  // (no stamped build of the stationary shape)
    if (pa.debug & 16) {
        n_waves = (size_t) 16 * ((call.batch + 1) / 2) * awpu::pair_tiles(h->cfg.pixel_count, h->pair_cols);
        if (const int rc = diag_begin(h, n_waves * 12, false, call.stream, &pa.debug_out); rc != AWPU_OK) return rc;
    }
    if (call.opts.timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, call.stream));
    if (!prepacked && !self_staged)
        AWPU_HIP_TRY(awpu::launch_pack_pairs(call.frames, h->cfg.n_streams, call.hist_eff, call.wstart_eff, h->d_index, h->usable(),
                                             h->usable(), nullptr, pp.wr, call.batch, h->d_pack, true, call.stream));  // gains ride on the table weights here
    const awpu::Extents have{plut->entries, prepacked ? prepacked_floats : h->d_pack.cap};
    if (stationary_tiles > 0) {
        AWPU_HIP_TRY(awpu::launch_das_pairs_stationary(pa, stationary_tiles, have, call.stream));
    } else {
        AWPU_HIP_TRY(awpu::launch_das_pairs(pa, have, call.stream));
    }
    return diag_end(h, finish_launch(h, call.batch, call.stream, call.opts.timed, stationary_tiles > 0 ? AWPU_KERNEL_PAIR_STATIONARY : AWPU_KERNEL_PAIR), n_waves, 16, "pairs", call.stream);
}

// quad shape: the frame-pair layout swept four vertically adjacent pixels at a time (das_quad_kernel)
int launch_quads(awpu_hip *h, const SweepCall &call, const float *prepacked = nullptr, size_t prepacked_floats = 0) {
    int rc = build_quad_lut(h, kQuadPairs);
    if (rc != AWPU_OK) return rc;
    const QuadTable &table = h->quad_tables[kQuadPairs];
    const awpu::FastPlan &pp = table.plan;
    if (!prepacked)
        if (const int prc = ensure_pack(h, pair_pack_floats(h->cfg.max_batch, pp.usable_pad, pp.wr, 2)); prc != AWPU_OK) return prc;
    awpu::QuadArgs qa{};
    fill_shared(qa, h, pp, call.batch, call.power);
    qa.packed = prepacked ? prepacked : h->d_pack;
    qa.lut = table.d;
    qa.wp = pp.wr;
    qa.cols = h->cfg.grid_columns;
    qa.rows = h->cfg.pixel_count / qa.cols;
    qa.tiles = awpu::quad_tiles(qa.rows, qa.cols);
    qa.n_pairs = (call.batch + 1) / 2;
    qa.pair_group = awpu::xcd_pair_group((size_t) pp.usable_pad * pp.wr * 8, qa.n_pairs, env().pair_group);
    qa.debug = env().debug;
    qa.variant = env().quad_variant;
    // Persistent workgroups (one per CU, each walking its share of the items with the next item's first chunk
    // prefetched) are 1.5 % faster than one workgroup per item on a chip they have to themselves, and fragile on one
    // they share: their share of the items is static.
    // Round 5: the persistent workgroups take their items from queues (one per XCD, a run's last eighth common to the chip) instead of
    // static shares -- balanced whatever the XCDs' clocks and whoever else holds CUs, so a rank's slab takes them too.
    // AWPU_FAST_WGS (tuning builds): that many workgroups on static shares; -1: one workgroup per item everywhere
    qa.wgs = std::max(0, env().wgs);
    if (env().wgs == 0)
        if (rc = arm_item_queues(h, qa.n_pairs * qa.tiles, &qa.queue, &qa.wgs, &qa.tail); rc != AWPU_OK) return rc;
    size_t n_waves = 0;
    if (qa.debug & 16) {
        const long per_xcd = ((long) qa.n_pairs * qa.tiles + 7) / 8;
        n_waves = (size_t) 16 * 8 * (size_t) (qa.wgs > 0 ? std::min<long>(per_xcd, std::max(1, qa.wgs / 8)) : per_xcd);
        if (rc = diag_begin(h, n_waves * 12, true, call.stream, &qa.debug_out); rc != AWPU_OK) return rc;
    }
    if (call.opts.timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, call.stream));
    if (!prepacked)
        AWPU_HIP_TRY(awpu::launch_pack_pairs(call.frames, h->cfg.n_streams, call.hist_eff, call.wstart_eff, h->d_index, h->usable(),
                                             pp.usable_pad, h->d_gain, pp.wr, call.batch, h->d_pack, true, call.stream));
    AWPU_HIP_TRY(awpu::launch_das_quads(qa, {table.entries, prepacked ? prepacked_floats : h->d_pack.cap}, call.stream));
    return diag_end(h, finish_launch(h, call.batch, call.stream, call.opts.timed, AWPU_KERNEL_QUAD), n_waves, 16, "quads", call.stream);
}

// quad shape for single frames on the halves layout (das_quadh_kernel): a pack + filter pre-pass, then the sweep
int launch_quadsh(awpu_hip *h, const SweepCall &call, int qpw) {
    int rc = build_quad_lut(h, kQuadHalves);
    if (rc != AWPU_OK) return rc;
    const QuadTable &table = h->quad_tables[kQuadHalves];
    const awpu::FastPlan &pp = table.plan;
    const size_t need = std::max((size_t) h->cfg.max_batch, (size_t) call.batch) * pp.usable_pad * pp.wr * 2;
    if (const int prc = ensure_pack(h, need); prc != AWPU_OK) return prc;
    awpu::QuadhArgs qa{};
    fill_shared(qa, h, pp, call.batch, call.power);
    qa.packed = h->d_pack;
    qa.lut = table.d;
    qa.wp = pp.wr;
    qa.cols = h->cfg.grid_columns;
    qa.rows = h->cfg.pixel_count / qa.cols;
    qa.debug = env().debug;
    size_t n_waves = 0;
    if (qa.debug & 16) {
        n_waves = (size_t) 16 * call.batch * awpu::quad1_tiles(qa.rows, qa.cols, qpw);
        if (rc = diag_begin(h, n_waves * 12, false, call.stream, &qa.debug_out); rc != AWPU_OK) return rc;
    }
    if (call.opts.timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, call.stream));
    AWPU_HIP_TRY(awpu::launch_pack_halves(call.frames, h->cfg.n_streams, call.hist_eff, call.hist_ring(), call.wstart_eff, h->identity_mics ? nullptr : h->d_index, h->usable(),
                                          pp.usable_pad, h->d_gain, pp.wr, call.batch, h->d_pack, call.stream));
    AWPU_HIP_TRY(awpu::launch_das_quadh(qa, qpw, {table.entries, h->d_pack.cap}, call.stream));
    return diag_end(h, finish_launch(h, call.batch, call.stream, call.opts.timed, AWPU_KERNEL_QUADH), n_waves, 16, "quadsh", call.stream);
}

// single frames of small arrays: every mic's halves row resident, the workgroup stages the window itself (das_quadh_stationary_kernel)
int launch_quadsh_stationary(awpu_hip *h, const SweepCall &call, int qpw) {
    int rc = build_quad_lut(h, kQuadHalvesStationary);
    if (rc != AWPU_OK) return rc;
    const QuadTable &table = h->quad_tables[kQuadHalvesStationary];
    const awpu::FastPlan &pp = table.plan;
    awpu::QuadhStationaryArgs qa{};
    qa.frames = call.frames;
    qa.lut = table.d;
    qa.index = h->d_index;
    qa.gain = h->d_gain;
    qa.power = call.power;
    qa.n_streams = h->cfg.n_streams;
    qa.pitch = call.hist_eff;
    qa.hist = call.hist_ring();
    qa.wstart = call.wstart_eff;
    qa.usable = h->usable();
    qa.usable_pad = pp.usable_pad;
    qa.pixel_count = h->cfg.pixel_count;
    qa.wp = pp.wr;
    qa.batch = call.batch;
    qa.cols = h->cfg.grid_columns;
    qa.rows = h->cfg.pixel_count / qa.cols;
    qa.waves = 16;
    qa.identity = h->identity_mics;
    qa.row_limit = call.hist_eff;  // (the ring's rows are 2048 floats of which any 1024 + window are valid: double-written)
    if (!awpu::quadh_stationary_raw(pp, qa.usable, call.wstart_eff, qa.row_limit, &qa.raw_begin, &qa.raw_wr, &qa.image_offset))
        return invalid("the raw window does not fit the LDS beside the halves image");  // (launch() asks before it comes here)
    if (call.opts.flag && call.stream == h->stream && qpw == 1) {  // (the one-frame host call: live_host_call)
        if (rc = arm_done_flag(h, (unsigned long long) call.batch * awpu::quad1_tiles(qa.rows, qa.cols, 1), &qa.done); rc != AWPU_OK) return rc;
    }
    if (call.opts.timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, call.stream));
    AWPU_HIP_TRY(awpu::launch_das_quadh_stationary(qa, qpw, {table.entries, 0}, call.stream));
    if (qa.done.flag) done_flag_armed(h, qa.done, call.opts.flag);
    return finish_launch(h, call.batch, call.stream, call.opts.timed, AWPU_KERNEL_QUADH_STATIONARY);
}

// single frames, whatever the table says: the 8-wave shape, or the double-buffered 16-wave one (das_fast_kernel / das_fast_db_kernel)
int launch_single(awpu_hip *h, const SweepCall &call, int fpi, int ppw, int nw) {
    const awpu_hip::FastLut *lut = nullptr;
    int rc = build_fast_lut(h, awpu::PackLayout::kSingle, fpi, awpu::fast_image_bytes(nw), &lut);
    if (rc != AWPU_OK) return rc;
    const awpu::FastPlan &plan = lut->plan;
    awpu::FastArgs a{};
    fill_shared(a, h, plan, call.batch, call.power);
    a.frames = call.frames;
    a.lut = lut->d;
    a.index = h->d_index;
    a.row_off = call.layout == kCompact ? h->d_row_off_compact : (call.layout == kRing ? h->d_row_off_ring : h->d_row_off);
    a.n_streams = h->cfg.n_streams;
    a.hist = call.hist_eff;
    a.wstart = call.wstart_eff;
    a.wr = plan.wr;
    // frames per persistent workgroup: measured, persistence over frames buys nothing
    a.frames_per_wg = std::min(env().fpw > 0 ? env().fpw : 1, call.batch);
    a.debug = env().debug;
    size_t n_waves = 0;
    const int wg_waves = nw == 24 ? 12 : 16;
    if ((a.debug & 16) && nw != 8) {  // the double-buffered shapes have a stamped build
        n_waves = (size_t) wg_waves * ((call.batch + a.frames_per_wg - 1) / a.frames_per_wg) *
                  ((h->cfg.pixel_count + wg_waves * ppw - 1) / (wg_waves * ppw));
        if (rc = diag_begin(h, n_waves * 12, false, call.stream, &a.debug_out); rc != AWPU_OK) return rc;
    }
    if (call.opts.timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, call.stream));
    AWPU_HIP_TRY(awpu::launch_das_fast(a, fpi, ppw, nw, {lut->entries, 0}, call.stream));
    const int id = nw == 32 ? AWPU_KERNEL_SINGLE_DB : (nw == 8 && fpi == 1 && ppw <= 4 ? AWPU_KERNEL_SINGLE_SMALL : AWPU_KERNEL_TUNING);
    return diag_end(h, finish_launch(h, call.batch, call.stream, call.opts.timed, id), n_waves, wg_waves, "single", call.stream);
}

// ---- the dispatch rule.  Its predicates first: launch() and the packed-frame entry points ask the same ones.

// Does a batch of AWPU_MATH_F32_FAST fill the chip with the quad shape (das_quad_kernel)?  (AWPU_SHAPE=quad: everywhere the table allows)
bool fast_batch_takes_quads(awpu_hip *h, int batch) {
    return h->quad_ok && env().pairs != 0 &&
           ((long) awpu::quad_tiles(h->cfg.pixel_count / h->cfg.grid_columns, h->cfg.grid_columns) * ((batch + 1) / 2) >= 256 || env().quads == 1);
}

// ... and are the quad shape's packed rows those of `plan` (a caller's packed frames: no padding rows)?
bool quad_plan_is(const awpu_hip *h, const awpu::FastPlan &plan) {
    const awpu::FastPlan &quad = h->quad_tables[kQuadPairs].plan;
    return quad.wr == plan.wr && quad.usable_pad == h->usable();
}

// ... with the pair shape (das_pair_kernel)?  (AWPU_SHAPE=pair: everywhere)
bool fast_batch_takes_pairs(awpu_hip *h, int batch) {
    return env().pairs != 0 && ((long) awpu::pair_tiles(h->cfg.pixel_count, h->pair_cols) * ((batch + 1) / 2) >= 256 || env().pairs == 1);
}

// one member per launcher and form of it that reports a kernel id of its own; kShapeNone: the call cannot be served
enum Shape { kShapeNone, kShapeFir8Planes, kShapeExactNdp, kShapeExactNdh, kShapeExactNd, kShapeExactQuads, kShapeExactPairs, kShapeExact,
             kShapeQuads, kShapePairsStationary, kShapePairs, kShapeQuadsh, kShapeQuadshStationary, kShapeSingle };
struct ShapeChoice {
    Shape shape;
    int nq = 1;               // exact quad kernels: quads per wave
    bool stationary = false;  // kShapeExactNdh: every mic resident, no pack pre-pass
    int qpw = 1;              // halves layout: quads per wave
    int tiles_per_wg = 0;     // kShapePairsStationary
    int fpi = 1, ppw = 0, nw = 0;  // kShapeSingle: frames per item, pixels per wave, 8 / 32 (choose_fast_variant)
};

// Which kernel sweeps `batch` frames of `layout`?  Decides only: no table is built, and the device is asked nothing but its CU count.
ShapeChoice choose_shape(awpu_hip *h, int batch, int layout, int hist_eff, int wstart_eff, const float *sums) {
    const auto &c = h->cfg;
    const int U = h->usable(), P = c.pixel_count, cols = c.grid_columns;
    const int rows = cols >= 1 ? P / cols : 0;
    const int n_pairs = (batch + 1) / 2;
    // FIR8 with fast math on a launch that fills the chip: the frame-pair kernels.  A single frame (or the odd last
    // one) is swept as a pair with itself -- half the packed lanes idle, still 1.6 x the rate of das_fir8_kernel.
    const long fir_wgs = (long) ((P + 63) / 64) * n_pairs;
    if (h->fir_planes_ok && env().pairs != 0 && env().fir_planes &&
        (fir_wgs >= (batch >= 2 ? 256 : 192) || (env().fir_planes == 2 && batch >= 2)))
        return {kShapeFir8Planes};
    const ExactShape ex = env().exact_pairs;
    if (h->exact_pairs_ok && ex != ExactShape::kVerify) {
        // vertical pixel quads on the {next, d} layout (round 5) where the row length is known and the table's statistics favour them
        // (takes_exact_nd; AWPU_SHAPE=exact_quad: round 4's kernel on raw sample pairs; exact_pair: the two-pixel block everywhere)
        int nq = 1;
        const bool nd = takes_exact_nd(h, batch, &nq);
        // one frame per call (MIMOWorker::update's regime): the halves form of the layout -- the two packed lanes are the two halves of
        // the block, not a frame and its copy; every mic resident where one array's rows fit the LDS (no pre-pass)
        const bool grid_known = cols >= 1 && P % cols == 0;
        if (batch == 1 && (ex == ExactShape::kDefault || ex == ExactShape::kNdp) && grid_known && (h->exact_ndhs_ok || h->exact_ndh_ok)) {
            // grids of at most 32 pixels per CU (two rounds of 16-wave workgroups): one PIXEL per wave (das_exact_ndp_kernel) -- a quad
            // kernel leaves such a grid one or two waves per SIMD, and the frame then takes as long as one wave's instruction issue.
            // Measured, 256 mics, one frame per call, quads -> pixels: 64 x 64 69.1 -> 31.6 us; 72^2 69.3 -> 52.1; 80^2 67.2 -> 53.3;
            // 88^2 66.1 -> 56.5; 96^2 (a third round) 81.1 -> 76.4; 100^2 69.3 -> 77.9 (profiles/r05_single_frame_ablation.txt).  It shares
            // no reads between pixels, so it also serves tables whose quads do not share (where the quad kernels are not chosen at all)
            // One array (every mic resident in the quad kernel, no pre-pass) against pixels behind the pre-pass: 32^2 (its quads do not
            // share: das_exact_pair_kernel) 36.9 -> 10.4 us; 48^2 22.3 -> 10.8; 64^2 21.1 -> 11.5; 80^2 20.3 -> 18.6; 100^2 (three rounds) 21.3 -> 26.0
            bool solo = h->exact_ndh_ok && awpu::ndp_tiles(rows, cols) * (long) batch <= 2L * cu_count(h);
            if (ex == ExactShape::kNdp) solo = h->exact_ndh_ok;
#ifdef AWPU_TUNING_BUILD
            if (const char *v = std::getenv("AWPU_NDH_WAVES")) solo = std::atoi(v) == 1 && h->exact_ndh_ok;
#endif
            if (solo) return {kShapeExactNdp};
            // (smaller workgroups of quads -- 8 or 4 waves, one round -- were the first answer to such grids: c2 76.6 -> 71.7 / 68.9 us;
            // one pixel per wave replaced them)
            if (nd) return {kShapeExactNdh, (long) awpu::quad1_tiles(rows, cols, 2) >= 256 ? 2 : 1, h->exact_ndhs_ok};
        }
        if (nd) return {kShapeExactNd, nq};
        if (ex == ExactShape::kQuad && h->pair_cols > 0 && rows >= 4) return {kShapeExactQuads};
        return {kShapeExactPairs};
    }
    // (the pre-epilogue sums: the frame-pair reference-order kernels above and das_fir8_kernel with the reference's rounding only)
    if (sums && !(c.math == AWPU_MATH_F32_EXACT && c.interp == AWPU_INTERP_FIR8)) return {kShapeNone};
    if (c.math != AWPU_MATH_F32_FAST || c.interp == AWPU_INTERP_FIR8) return {kShapeExact};

    // ---- frame-pair shapes: batches on grids that fill the chip (AWPU_FAST_PAIRS=0/1 overrides), never off the ring
    const bool pairable = layout != kRing && batch >= 2;
    if (pairable && fast_batch_takes_quads(h, batch)) return {kShapeQuads};
    // ---- stationary shape: the whole window of every active mic of a frame pair fits the LDS (one 8x8 array does)
    awpu::FastPlan plan;
    if (pairable && env().pairs != 0 && env().stationary != 0 && awpu::pair_plan_stationary(h->window, U, &plan)) {
        const long tiles = awpu::pair_tiles(P, h->pair_cols);
        if (n_pairs * tiles >= 128 || env().stationary == 1) {
            // tiles per workgroup: enough to amortise the staging, few enough to leave every CU a workgroup
#ifndef AWPU_STATIONARY_WGS
#define AWPU_STATIONARY_WGS 256  // (tuning builds: -DAWPU_STATIONARY_WGS=512 ... through tools/build_variant.sh)
#endif
            ShapeChoice choice{kShapePairsStationary};
            choice.tiles_per_wg = (int) std::max<long>(1, std::min<long>(tiles, n_pairs * tiles / AWPU_STATIONARY_WGS));
            return choice;
        }
    }
    // (a window too wide for the pair image is served by the single-frame shapes below)
    if (pairable && fast_batch_takes_pairs(h, batch) && awpu::pair_plan(h->window, U, &plan)) return {kShapePairs};
    // ---- single frames on grids of at most 16 pixels per CU: the reference-order kernel with one pixel per wave
    // (das_exact_ndp_kernel) is the fastest sweep this library has for them in ANY mode (c2, one frame per call: 47.6 us on this
    // mode's 8-wave shape, 29.9 us there; c1 11.7 -> 10.1) and its powers are the reference's own arithmetic -- inside this
    // mode's contract on any input.  Not when a shape of this mode is forced (AWPU_SHAPE: the tests sweep each through the oracle)
    if (h->fast_ndp_ok && cols >= 1 && P % cols == 0 && env().fpi == 0 && env().halves == -1 && env().quads == -1 && env().pairs == -1 &&
        env().stationary == -1 && awpu::ndp_tiles(rows, cols) * (long) batch <= cu_count(h))
        return {kShapeExactNdp};
    // ---- single frames on a grid whose table favours the quad shape (a forced single-frame shape goes past): the halves
    // layout behind a pack + filter pre-pass
    if (h->quadh_fits && env().fpi == 0 && env().halves != 0) {
        ShapeChoice choice{kShapeQuadsh};
        choice.qpw = (long) awpu::quad1_tiles(rows, cols, 2) * batch >= 256 ? 2 : 1;
        const long wgs = (long) awpu::quad1_tiles(rows, cols, choice.qpw) * batch;
        const bool forced = env().quads == 1 || env().halves == 1;
        // one 8x8 array (every mic's halves row fits the LDS): one launch, no pack pre-pass, no chunks.  A call this small is
        // latency, not throughput: taken from 48 workgroups on (below that the 8-wave shapes spread a tiny grid over more CUs)
        int rb = 0, rw = 0, io = 0;
        if (h->quadhs_fits && env().stationary != 0 && (wgs >= 48 || forced || env().stationary == 1) &&
            awpu::quadh_stationary_raw(h->quad_tables[kQuadHalvesStationary].plan, U, wstart_eff, hist_eff, &rb, &rw, &io)) {
            choice.shape = kShapeQuadshStationary;
            return choice;
        }
        // from 96 workgroups on.  (Measured, one frame per call, 256 mics: a 100 x 100 grid = 175 workgroups 54.5 us here against
        // 98.9 us for the 8-wave shape; 64 x 64 = 64 workgroups 56.5 against 47.8 -- this kernel's time is its 256-stage
        // dependent chain whatever the grid, the 8-wave shape's grows with the pixels: they cross near 80 workgroups.  The
        // threshold of rounds 2-3 was 192 and sent the four-array, default-resolution case to the slower shape.)
        if (wgs >= 96 || forced) return choice;
    }
    ShapeChoice choice{kShapeSingle};
    choose_fast_variant(h, batch, &choice.fpi, &choice.ppw, &choice.nw);
    // the double-buffered shapes read whole 16-byte pieces of every staged row
    if (choice.nw != 8 && !(awpu::fast_plan(h->window, U, choice.fpi, awpu::fast_image_bytes(choice.nw), &plan) && awpu::fast_db_fits(plan) &&
                            wstart_eff + 1 + plan.wr <= hist_eff)) {
        choice.nw = 8;
        if (choice.ppw > 4) choice.ppw = 4;  // (the 8-wave shape is built for 2 and 4 pixels per wave)
    }
    return choice;
}

}  // namespace

namespace awpu::host {

int launch(awpu_hip *h, const float *d_frames, int batch, float *d_power, hipStream_t s, int layout, const SweepOpts &o) {
    const int hist_eff = layout == kCompact ? h->compact_hist : (layout == kRing ? 2048 : h->cfg.hist);
    const SweepCall call{d_frames, batch, d_power, s, layout, hist_eff, layout == kCompact ? 0 : h->wstart, o};
    const ShapeChoice c = choose_shape(h, batch, layout, hist_eff, call.wstart_eff, o.sums);
    const awpu_hip::FastLut *lut = nullptr;
    switch (c.shape) {
    case kShapeFir8Planes: return launch_fir8_planes(h, call);
    case kShapeExactNdp: return launch_exact_ndh(h, call, false, 1, true);
    case kShapeExactNdh: return launch_exact_ndh(h, call, c.stationary, c.nq);
    case kShapeExactNd: return launch_exact_nd(h, call, c.nq);
    case kShapeExactQuads: return launch_exact_quads(h, call);
    case kShapeExactPairs: return launch_exact_pairs(h, call);
    case kShapeExact: return launch_exact(h, call);
    case kShapeQuads: return launch_quads(h, call);
    case kShapePairsStationary:
        if (const int rc = build_fast_lut(h, awpu::PackLayout::kPairsStationary, 2, 0, &lut); rc != AWPU_OK) return rc;
        return launch_pairs(h, lut, call, c.tiles_per_wg);
    case kShapePairs:
        if (const int rc = build_fast_lut(h, awpu::PackLayout::kPairs, 2, 0, &lut); rc != AWPU_OK) return rc;
        return launch_pairs(h, lut, call);
    case kShapeQuadsh: return launch_quadsh(h, call, c.qpw);
    case kShapeQuadshStationary: return launch_quadsh_stationary(h, call, c.qpw);
    case kShapeSingle: return launch_single(h, call, c.fpi, c.ppw, c.nw);
    case kShapeNone: break;
    }
    return fail(AWPU_ERR_STATE, "the pre-epilogue sums are exported by the frame-pair reference-order kernels and the reference-rounding FIR8 kernel only");
}

// The coherence sweep's table on a prepared handle whose prepare() built no d_lut (AWPU_MATH_F32_FAST with AWPU_INTERP_LERP): the
// same entries into d_cohere_lut, once per prepare() (free_tables drops it).  The copy blocks, so every coherence call comes here
// behind check_ready and before it enqueues anything; a copy that fails leaves no table behind, and the next call builds it again.
int ensure_cohere_table(awpu_hip *h) {
    if (h->d_lut || h->d_cohere_lut) return AWPU_OK;
    const int U = h->usable(), P = h->cfg.pixel_count;
    if (awpu::das_exact_lds_bytes(h->window, U, nullptr) == 0) return invalid("delay window does not fit the LDS budget");
    std::vector<awpu::LutEntry> packed((size_t) P * U);
    for (int p = 0; p < P; p++)
        for (int k = 0; k < U; k++) {
            const size_t at = (size_t) p * h->cfg.lut_stride + h->index[k];
            packed[(size_t) p * U + k] = {h->off[at] - h->wstart, h->frac[at]};
        }
    if (const int rc = h->d_cohere_lut.grow(packed.size()); rc != AWPU_OK) return rc;
    const hipError_t e = hipMemcpy(h->d_cohere_lut, packed.data(), packed.size() * sizeof(awpu::LutEntry), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        h->d_cohere_lut.release();
        return hip_fail(e, "hipMemcpy of the coherence sweep's table");
    }
    return AWPU_OK;
}

// The coherence sweep (awpu_hip_cohere.h; cohere_sweep_kernel), beside launch_exact: das_exact_kernel's arguments in the layouts
// launch() takes (kFull, kCompact), whatever cfg.math is -- the rule has one arithmetic.  Its table is d_lut where prepare() built
// it (every mode but AWPU_MATH_F32_FAST), else the same entries in d_cohere_lut (ensure_cohere_table).  Each output or null;
// counted and timed like any sweep launch.  Nothing here waits for the device.
int launch_cohere(awpu_hip *h, const float *d_frames, int batch, const CohereOut &out, hipStream_t s, int layout, bool timed) {
    if (h->cfg.interp != AWPU_INTERP_LERP) return fail(AWPU_ERR_STATE, "the coherence sweep interpolates linearly: AWPU_INTERP_FIR8 is not taken");
    if (layout != kFull && layout != kCompact) return invalid("the coherence sweep takes whole frames or uploaded windows");
    const int U = h->usable(), P = h->cfg.pixel_count;
    const awpu::LutEntry *lut = h->d_lut ? h->d_lut.get() : h->d_cohere_lut.get();
    if (!lut) return fail(AWPU_ERR_STATE, "the coherence sweep has no table: ensure_cohere_table comes first");
    awpu::CohereArgs a{};
    a.sweep.frames = d_frames;
    a.sweep.lut = lut;
    a.sweep.index = h->d_index;
    a.sweep.power = out.power;
    a.sweep.gain = h->d_gain;
    a.sweep.sums = out.sums;
    a.sweep.n_streams = h->cfg.n_streams;
    a.sweep.hist = layout == kCompact ? h->compact_hist : h->cfg.hist;
    a.sweep.usable = U;
    a.sweep.pixel_count = P;
    a.sweep.wstart = layout == kCompact ? 0 : h->wstart;
    a.sweep.window = h->window;
    a.sweep.batch = batch;
    a.coherence = out.coherence;
    a.weighted = out.weighted;
    a.energy = out.energy;
    if (timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, s));
    AWPU_HIP_TRY(awpu::launch_cohere_sweep(a, s));
    return finish_launch(h, batch, s, timed, AWPU_KERNEL_COHERE);
}

// The tone sweep's two tables (awpu_hip_tones.h), from the library's own host functions: both windows, then the twiddles, once per
// handle.  The copy blocks, so every tone call comes here beside ensure_cohere_table, before it enqueues anything.
int ensure_tones_tables(awpu_hip *h) {
    if (h->d_tones_tables) return AWPU_OK;
    std::vector<float> tables(3 * awpu::kSamples);
    awpu_hip_tones_window(AWPU_TONES_RECT, tables.data());
    awpu_hip_tones_window(AWPU_TONES_HANN, tables.data() + awpu::kSamples);
    awpu_hip_tones_twiddles(reinterpret_cast<float(*)[2]>(tables.data() + 2 * awpu::kSamples));
    if (const int rc = h->d_tones_tables.grow(tables.size()); rc != AWPU_OK) return rc;
    const hipError_t e = hipMemcpy(h->d_tones_tables, tables.data(), tables.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        h->d_tones_tables.release();
        return hip_fail(e, "hipMemcpy of the tone sweep's tables");
    }
    return AWPU_OK;
}

// The tone sweep (awpu_hip_tones.h; tones_sweep_kernel), beside launch_cohere and with its arguments, table and layouts: whatever
// cfg.math is, the rule has one arithmetic.  `t` has passed tones_refusal; it travels as a kernel argument.  Each output or null;
// counted and timed like any sweep launch.  Nothing here waits for the device.
int launch_tones(awpu_hip *h, const float *d_frames, int batch, const awpu_tones_t &t, const TonesOut &out, hipStream_t s, int layout, bool timed) {
    if (h->cfg.interp != AWPU_INTERP_LERP) return fail(AWPU_ERR_STATE, "the tone sweep interpolates linearly: AWPU_INTERP_FIR8 is not taken");
    if (layout != kFull && layout != kCompact) return invalid("the tone sweep takes whole frames or uploaded windows");
    const awpu::LutEntry *lut = h->d_lut ? h->d_lut.get() : h->d_cohere_lut.get();
    if (!lut || !h->d_tones_tables) return fail(AWPU_ERR_STATE, "the tone sweep has no tables: ensure_cohere_table and ensure_tones_tables come first");
    awpu::TonesArgs a{};
    a.sweep.frames = d_frames;
    a.sweep.lut = lut;
    a.sweep.index = h->d_index;
    a.sweep.gain = h->d_gain;
    a.sweep.n_streams = h->cfg.n_streams;
    a.sweep.hist = layout == kCompact ? h->compact_hist : h->cfg.hist;
    a.sweep.usable = h->usable();
    a.sweep.pixel_count = h->cfg.pixel_count;
    a.sweep.wstart = layout == kCompact ? 0 : h->wstart;
    a.sweep.window = h->window;
    a.sweep.batch = batch;
    a.window = h->d_tones_tables.get() + (t.window == AWPU_TONES_HANN ? awpu::kSamples : 0);
    a.twiddles = h->d_tones_tables.get() + 2 * awpu::kSamples;
    a.wss = t.window == AWPU_TONES_HANN ? 96.0f : 256.0f;
    a.tone = out.tone;
    a.pitch = out.pitch;
    a.pitch_row = out.pitch_row;
    a.bins = out.bins;
    a.spectrum = out.spectrum;
    a.t = t;
    if (timed) AWPU_HIP_TRY(hipEventRecord(h->ev_begin, s));
    AWPU_HIP_TRY(awpu::launch_tones_sweep(a, s));
    return finish_launch(h, batch, s, timed, AWPU_KERNEL_TONES);
}

// Would launch() sweep this batch with one of the frame-pair shapes that read the packed layout (quad or pair)?  The rule of
// awpu_hip_process_packed, asked before anything is packed.
bool takes_packed_pairs(awpu_hip *h, int batch, awpu::FastPlan *plan) {
    if (batch < 2 || h->cfg.interp != AWPU_INTERP_LERP || h->usable() % 4 != 0 || !h->gain.empty()) return false;
    if (h->cfg.math == AWPU_MATH_F32_EXACT) {  // the reference's order: the {next, d} rows of das_exact_nd_kernel
        int nq = 1;
        if (!takes_exact_nd(h, batch, &nq)) return false;
        *plan = h->quad_tables[kQuadExactNd].plan;
        return true;
    }
    if (h->cfg.math != AWPU_MATH_F32_FAST || env().pairs == 0) return false;
    if (!awpu::pair_plan(h->window, h->usable(), plan)) return false;
    return (fast_batch_takes_quads(h, batch) && quad_plan_is(h, *plan)) || fast_batch_takes_pairs(h, batch);
}

// floats of `batch` frames in the packed layout of `plan` (rows of plan.row_bytes: sample pairs of a frame pair, or their {next, d}
// elements), `usable` rows per pair (the packed entry points ask for usable % 4 == 0: no padding rows)
size_t packed_floats_of(const awpu_hip *h, const awpu::FastPlan &plan, int batch) {
    // (the {next, d} plan's row_bytes is its LDS row, the tile window; its packed rows hold wr elements of four floats)
    return (size_t) ((batch + 1) / 2) * h->usable() * (size_t) (plan.layout == awpu::PackLayout::kNd ? plan.wr * 4 : plan.row_bytes / 4);
}

// the sweep's pack pass into a caller's buffer: pre-filtered sample pairs (FAST) or {next, d} elements (EXACT)
int pack_for_sweep(awpu_hip *h, const awpu::FastPlan &plan, const float *d_frames, int batch, float *d_packed, hipStream_t s) {
    if (h->cfg.math == AWPU_MATH_F32_EXACT)
        AWPU_HIP_TRY(awpu::launch_pack_nd(d_frames, h->cfg.n_streams, h->cfg.hist, h->wstart, h->d_index, h->usable(), h->usable(), nullptr, plan.wr,
                                          batch, d_packed, nullptr, s));
    else
        AWPU_HIP_TRY(awpu::launch_pack_pairs(d_frames, h->cfg.n_streams, h->cfg.hist, h->wstart, h->d_index, h->usable(), h->usable(), nullptr,
                                             plan.wr, batch, d_packed, true, s));
    return AWPU_OK;
}

// The sweep of packed frame pairs (what awpu_hip_process_packed does once its arguments are checked): the shape launch() takes for
// this batch, as long as that is a frame-pair shape -- launch()'s own predicates, so the same bits.  The buffer is the caller's, so
// never the stationary shape (it stages from the frames), and the quad shape only where its rows are the packed plan's.
int sweep_packed(awpu_hip *h, const awpu::FastPlan &plan, const float *d_packed, size_t packed_floats, int batch, float *d_power,
                 hipStream_t s) {
    const SweepCall call{nullptr, batch, d_power, s, kFull, h->cfg.hist, h->wstart, {}};  // (every caller is asynchronous: untimed)
    if (h->cfg.math == AWPU_MATH_F32_EXACT) {
        int nq = 1;
        if (!takes_exact_nd(h, batch, &nq)) return fail(AWPU_ERR_STATE, "packed frames: this batch is not swept by the {next, d} kernel");
        return launch_exact_nd(h, call, nq, d_packed, packed_floats);
    }
    if (fast_batch_takes_quads(h, batch) && quad_plan_is(h, plan)) return launch_quads(h, call, d_packed, packed_floats);
    const awpu_hip::FastLut *plut = nullptr;
    const int rc = build_fast_lut(h, awpu::PackLayout::kPairs, 2, 0, &plut);
    if (rc != AWPU_OK) return rc;
    return launch_pairs(h, plut, call, 0, d_packed, packed_floats);
}

// The layout both frame-pair shapes read when usable is a multiple of four and no gains are set:
// [ceil(batch/2)][usable][wr][2] floats.  AWPU_ERR_STATE when this handle's sweep does not take packed frames.
int packed_shape(awpu_hip *h, int batch, awpu::FastPlan *plan) {
    if ((h->cfg.math != AWPU_MATH_F32_FAST && h->cfg.math != AWPU_MATH_F32_EXACT) || h->cfg.interp != AWPU_INTERP_LERP)
        return fail(AWPU_ERR_STATE, "packed frames need AWPU_MATH_F32_EXACT or AWPU_MATH_F32_FAST, and AWPU_INTERP_LERP");
    if (h->usable() % 4 != 0 || !h->gain.empty())
        return fail(AWPU_ERR_STATE, "packed frames need usable % 4 == 0 and no mic gains (the shapes of a mode then read one layout)");
    if (h->cfg.math == AWPU_MATH_F32_EXACT) {  // the {next, d} rows of das_exact_nd_kernel: where launch() takes that kernel for this batch
        int nq = 1;
        if (batch < 2 || !takes_exact_nd(h, batch, &nq))
            return fail(AWPU_ERR_STATE, "packed frames in the reference's order need the grid's row length (grid_columns) and a batch of two or more");
        *plan = h->quad_tables[kQuadExactNd].plan;
        return AWPU_OK;
    }
    if (!awpu::pair_plan(h->window, h->usable(), plan)) return fail(AWPU_ERR_STATE, "the window does not fit the frame-pair image");
    return AWPU_OK;
}

}  // namespace awpu::host
