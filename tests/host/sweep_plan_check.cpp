// The planners of the sweep kernels' LDS images (csrc/sweep_plan.h), with no device: every planner on seven (window, usable) inputs
// against the plans recorded from the library before the planners moved into the header; the layout each planner names; and the XCD
// pair group of the FIR8 plane launch against the rule its launcher used to write out itself.  Prints "ok" and exits 0, or says
// what differs.
#include <algorithm>
#include <cstddef>
#include <cstdio>

#include "sweep_plan.h"

using awpu::FastPlan;
using awpu::PackLayout;

namespace {

struct Want {
    int ok, fpi, wr, chunk, usable_pad, row_bytes;
};
constexpr Want kNo = {0, 0, 0, 0, 0, 0};
constexpr int kInputs = 7;
constexpr int kWindow[kInputs] = {285, 285, 348, 355, 257, 1024, 5000}, kUsable[kInputs] = {64, 51, 256, 512, 1, 256, 64};

struct Row {
    const char *name;
    bool (*plan)(int window, int usable, FastPlan *plan);
    PackLayout layout;
    Want want[kInputs];
};
const Row kRows[] = {
    {"pair", [](int w, int u, FastPlan *p) { return awpu::pair_plan(w, u, p); }, PackLayout::kPairs,
     {{1, 2, 286, 32, 64, 2288}, {1, 2, 286, 32, 52, 2288}, {1, 2, 348, 28, 256, 2784}, {1, 2, 356, 28, 512, 2848}, {1, 2, 258, 4, 4, 2064}, {1, 2, 1024, 8, 256, 8192}, kNo}},
    {"pair stationary", [](int w, int u, FastPlan *p) { return awpu::pair_plan_stationary(w, u, p); }, PackLayout::kPairsStationary,
     {{1, 2, 286, 64, 64, 2288}, {1, 2, 286, 52, 52, 2288}, kNo, kNo, {1, 2, 258, 4, 4, 2064}, kNo, kNo}},
    {"fir8 planes", [](int w, int u, FastPlan *p) { return awpu::fir8_plane_plan(w, u, p); }, PackLayout::kFir8Planes,
     {{1, 2, 288, 32, 64, 2304}, {1, 2, 288, 32, 52, 2304}, {1, 2, 384, 24, 256, 3072}, {1, 2, 384, 24, 512, 3072}, {1, 2, 260, 4, 4, 2080}, {1, 2, 1024, 8, 256, 8192}, kNo}},
    {"exact nd, wq_tile 0", [](int w, int u, FastPlan *p) { return awpu::exact_nd_plan(w, u, 0, p); }, PackLayout::kNd,
     {{1, 2, 284, 16, 64, 4544}, {1, 2, 284, 16, 52, 4544}, {1, 2, 347, 12, 256, 5552}, {1, 2, 354, 12, 512, 5664}, {1, 2, 256, 4, 4, 4096}, {1, 2, 1023, 4, 256, 16368}, kNo}},
    {"exact nd, wq_tile 279", [](int w, int u, FastPlan *p) { return awpu::exact_nd_plan(w, u, 279, p); }, PackLayout::kNd,
     {{1, 2, 284, 16, 64, 4464}, {1, 2, 284, 16, 52, 4464}, {1, 2, 347, 16, 256, 4464}, {1, 2, 354, 16, 512, 4464}, {1, 2, 256, 4, 4, 4096}, {1, 2, 1023, 16, 256, 4464},
      {1, 2, 4999, 16, 64, 4464}}},
    {"exact ndh chunked", [](int w, int u, FastPlan *p) { return awpu::exact_ndh_plan(w, u, false, p); }, PackLayout::kNdHalves,
     {{1, 1, 156, 32, 64, 2496}, {1, 1, 156, 32, 52, 2496}, {1, 1, 219, 20, 256, 3504}, {1, 1, 226, 20, 512, 3616}, {1, 1, 128, 4, 4, 2048}, {1, 1, 895, 4, 256, 14320}, kNo}},
    {"exact ndh stationary", [](int w, int u, FastPlan *p) { return awpu::exact_ndh_plan(w, u, true, p); }, PackLayout::kNdHalvesStationary,
     {{1, 1, 156, 64, 64, 2496}, {1, 1, 156, 52, 52, 2496}, kNo, kNo, {1, 1, 128, 4, 4, 2048}, kNo, kNo}},
    {"quadh stationary", [](int w, int u, FastPlan *p) { return awpu::quadh_stationary_plan(w, u, p); }, PackLayout::kHalvesStationary,
     {{1, 1, 158, 64, 64, 1264}, {1, 1, 158, 52, 52, 1264}, kNo, kNo, {1, 1, 130, 4, 4, 1040}, kNo, kNo}},
    {"fast, fpi 1, 78 KiB", [](int w, int u, FastPlan *p) { return awpu::fast_plan(w, u, 1, 78 * 1024, p); }, PackLayout::kSingle,
     {{1, 1, 288, 32, 64, 1152}, {1, 1, 288, 32, 52, 1152}, {1, 1, 348, 28, 256, 1392}, {1, 1, 356, 28, 512, 1424}, {1, 1, 260, 4, 4, 1040}, {1, 1, 1024, 8, 256, 4096}, kNo}},
};

// das_fir8_plane_kernel's launcher before it took PairArgs::pair_group: its own copy of the rule, verbatim
int old_fir8_pair_group(int usable, int wp, int n_pairs) {
    const size_t pair_bytes = (size_t) usable * wp * 8;
    int g = (int) std::max<size_t>(1, (3u << 20) / pair_bytes);
    g = g >= 8 ? 8 : g >= 4 ? 4 : g >= 2 ? 2 : 1;
    while (g > 1 && g > n_pairs) g >>= 1;
    return g;
}

}  // namespace

int main() {
    int bad = 0;
    for (const Row &row : kRows)
        for (int k = 0; k < kInputs; k++) {
            FastPlan p{};
            const Want &w = row.want[k];
            const bool ok = row.plan(kWindow[k], kUsable[k], &p);
            const bool same = ok ? w.ok == 1 && p.fpi == w.fpi && p.wr == w.wr && p.chunk == w.chunk && p.usable_pad == w.usable_pad && p.row_bytes == w.row_bytes
                                 : w.ok == 0;
            if (!same) {
                std::printf("%s, window %d, usable %d: %d/%d/%d/%d/%d/%d, recorded %d/%d/%d/%d/%d/%d\n", row.name, kWindow[k], kUsable[k], (int) ok, p.fpi,
                            p.wr, p.chunk, p.usable_pad, p.row_bytes, w.ok, w.fpi, w.wr, w.chunk, w.usable_pad, w.row_bytes);
                bad++;
            }
            if (ok && p.layout != row.layout) std::printf("%s: layout %d, not its own %d\n", row.name, (int) p.layout, (int) row.layout), bad++;
            // image_bytes keeps its literal meaning: the staged image of the single-frame shapes, nothing elsewhere
            if (ok && p.image_bytes != (row.layout == PackLayout::kSingle ? 78 * 1024 : 0)) std::printf("%s: image_bytes %d\n", row.name, p.image_bytes), bad++;
        }
    {   // the two layouts that shared a tag compare unequal
        FastPlan fir{}, halves{};
        if (!awpu::fir8_plane_plan(285, 64, &fir) || !awpu::quadh_stationary_plan(285, 64, &halves) || fir.layout == halves.layout)
            std::printf("the FIR8 plane layout and the stationary halves layout are one\n"), bad++;
    }
    for (int usable : {4, 64, 256, 512})
        for (int wr : {260, 288, 384, 1024})
            for (int n_pairs = 1; n_pairs <= 9; n_pairs++) {
                const int got = awpu::xcd_pair_group((size_t) usable * wr * 8, n_pairs), want = old_fir8_pair_group(usable, wr, n_pairs);
                if (got != want) std::printf("pair group, usable %d, wr %d, %d pairs: %d, the launcher's rule %d\n", usable, wr, n_pairs, got, want), bad++;
            }
    if (bad) std::printf("%d differences\n", bad);
    else std::printf("ok\n");
    return bad ? 1 : 0;
}
