// csm_run_plan.h by itself, under sanitizers (tests/test_csm_run_plan_cpu.py): the scratch totals recorded from the library before
// the run's arithmetic became this header, the layout's properties, the chunk walk by brute force and the frames' windows.
#include "csm_run_plan.h"

#include <cstdio>

using namespace awpu;

static int failures = 0;
#define CHECK(cond, ...)                                         \
    do {                                                         \
        if (!(cond)) {                                           \
            if (failures++ < 20) {                               \
                std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                        \
                std::printf("\n");                               \
            }                                                    \
        }                                                        \
    } while (0)

struct Row {
    int host, wire, S, U, K, P, keep, chunk, piece, planes, solved, steps, power, clean_steps;
};
static CsmRunShape shape_of(const Row &r) {
    return {r.host != 0, r.wire != 0, r.S, r.U, r.K, r.P, r.keep, r.chunk, r.piece, r.planes != 0, r.solved != 0, r.steps != 0, r.power != 0, r.clean_steps};
}

// the total in floats of the run's scratch as the run computed it inline, before this header: the literals were recorded from that expression
static const struct {
    Row in;
    size_t total;
} kRecorded[] = {
    // host wire S   U  K      P  keep chunk piece planes solved steps power clean_steps
    {{1, 1,   8,   5, 3,   256,    0,  11,  2, 1, 1, 0, 1,  0}, 751752u},
    {{1, 1,   8,   5, 3,   256,    6,  11,  2, 0, 0, 0, 1,  0}, 751336u},
    {{1, 1,  64,  64, 8,  1024,    4, 256,  8, 1, 0, 0, 0,  0}, 21577732u},
    {{1, 1, 256, 255, 1, 16384,   63, 256, 32, 0, 1, 0, 1,  0}, 34681140u},
    {{1, 1,   3,   1, 1,     9,    0,   1,  1, 0, 0, 0, 1,  0}, 66856u},
    {{1, 1,   8,   2, 1,    16,    2, 256,  2, 1, 0, 1, 1,  2}, 17433712u},
    {{1, 1,  64,  64, 3,    64,    4,  12,  2, 1, 0, 1, 1,  3}, 1046588u},
    {{1, 1,  64,  63, 5,   225,    0, 256,  1, 0, 0, 1, 0, 32}, 21345096u},
    {{1, 1,  64,  63, 5,   225,    9, 100,  7, 1, 0, 0, 1,  1}, 8406384u},
    {{1, 0,   8,   5, 3,   256,    0,  11,  2, 1, 1, 0, 1,  0}, 25220u},
    {{1, 0,   8,   5, 3,   256,   11,  11,  2, 0, 0, 0, 1,  0}, 25104u},
    {{1, 0,  64,  64, 8,  1024,    4, 256,  8, 1, 1, 0, 0,  0}, 4669504u},
    {{1, 0, 256, 255, 1, 16384,   63, 256, 32, 0, 1, 0, 1,  0}, 17772848u},
    {{1, 0,   3,   1, 1,     9,    0,   1,  1, 0, 0, 0, 1,  0}, 804u},
    {{1, 0,   7,   3, 7,    49,    1,   3,  1, 1, 1, 0, 1,  0}, 6248u},
    {{1, 0,   8,   2, 1,    16,    2, 256,  2, 1, 0, 1, 1,  2}, 525420u},
    {{1, 0,  64,  64, 3,    64,    4,  12,  2, 1, 0, 1, 1,  3}, 254008u},
    {{1, 0,  64,  63, 5,   225,    0, 256,  1, 0, 0, 1, 0, 32}, 4436804u},
    {{1, 0,  64,  63, 5,   225,    9, 100,  7, 1, 0, 0, 1,  1}, 1801580u},
    {{1, 0, 128,  65, 2, 10000, 1023, 256,  8, 0, 0, 1, 1, 32}, 9122464u},
    {{0, 0,   8,   5, 3,   256,    0,  11,  2, 1, 1, 0, 1,  0}, 636u},
    {{0, 0,   8,   5, 3,   256,    6,  11,  2, 0, 0, 0, 1,  0}, 1584u},
    {{0, 0,   8,   5, 3,   256,    6,  11,  2, 0, 1, 0, 0,  0}, 2096u},
    {{0, 0,  64,  64, 8,  1024,    4, 256,  8, 1, 0, 0, 0,  0}, 405504u},
    {{0, 0, 256, 255, 1, 16384,   63, 256, 32, 0, 1, 0, 1,  0}, 439180u},
    {{0, 0,   3,   1, 1,     9,    0,   1,  1, 0, 0, 0, 1,  0}, 24u},
    {{0, 0,   8,   2, 1,    16,    2, 256,  2, 1, 0, 1, 1,  2}, 1048u},
    {{0, 0,  64,  63, 5,   225,    0, 256,  1, 0, 0, 1, 0, 32}, 242020u},
    {{0, 0,  64,  63, 5,   225,    9, 100,  7, 1, 0, 0, 1,  1}, 148056u},
    {{0, 0,  64,  64, 8, 16384,   63,  64,  8, 0, 0, 0, 1,  0}, 392192u},
};

static void check_layout() {
    static_assert(sizeof(kRecorded) / sizeof(kRecorded[0]) >= 24, "the table");
    int row = 0;
    for (const auto &rec : kRecorded) {
        const Row &r = rec.in;
        const CsmRunLayout L = csm_run_layout(shape_of(r));
        CHECK(L.total == rec.total, "row %d: total %zu, recorded %zu", row, L.total, rec.total);
        // disjoint, in the order of the header, each on a multiple of 4 floats
        const CsmRunRegion *regions[] = {&L.spectra, &L.carry, &L.matrix, &L.second, &L.rows, &L.planes, &L.solved, &L.steps, &L.stage, &L.wire};
        size_t at = 0;
        for (const CsmRunRegion *g : regions) {
            CHECK(g->off == at && g->off % 4 == 0 && g->floats % 4 == 0, "row %d: a region at %zu of %zu floats behind %zu", row, g->off, g->floats, at);
            at += g->floats;
        }
        CHECK(at == L.total, "row %d", row);
        // every region holds what the run puts there ...
        const size_t K = r.K, U = r.U, P = r.P, piece = r.piece, per_block = K * U * 2;
        CHECK(L.spectra.floats >= (size_t) (r.keep + r.chunk) * per_block && L.matrix.floats >= K * U * U * 2 && L.second.floats == L.matrix.floats, "row %d", row);
        if (r.host) {
            CHECK(L.carry.floats >= (size_t) r.keep * per_block && L.rows.floats >= piece * P && L.stage.floats >= (size_t) r.S * 256 * r.chunk, "row %d", row);
            CHECK(L.planes.floats >= (r.planes ? piece : 1) * K * P, "row %d", row);
        }
        if (r.wire) CHECK(L.wire.floats * sizeof(float) >= (size_t) 256 * r.chunk * 1032, "row %d", row);
        // ... and a region nobody asked for is empty
        if (!r.host) CHECK(L.carry.floats == 0 && L.solved.floats == 0 && L.steps.floats == 0 && L.stage.floats == 0, "row %d", row);
        if (!r.host && r.power) CHECK(L.rows.floats == 0, "row %d", row);
        if (!r.host && r.planes) CHECK(L.planes.floats == 0, "row %d", row);
        if (!r.host && !r.planes) CHECK(L.planes.floats >= K * P, "row %d", row);
        if (!r.solved) CHECK(L.solved.floats == 0, "row %d", row);
        if (r.host && r.solved) CHECK(L.solved.floats >= piece * K, "row %d", row);
        if (!r.steps || r.clean_steps == 0) CHECK(L.steps.floats == 0, "row %d", row);
        if (r.host && r.steps) CHECK(L.steps.floats >= piece * K * r.clean_steps * 3, "row %d", row);
        if (!r.wire) CHECK(L.wire.floats == 0, "row %d", row);
        if (r.keep == 0) CHECK(L.carry.floats == 0, "row %d", row);
        row++;
    }
}

// the walk of one call, and the windows of its frames for every carried_in
static void check_walk(int n_blocks, int first, int every, int piece, int length) {
    const int keep = length - 1, n_frames = first < n_blocks ? (n_blocks - 1 - first) / every + 1 : 0;
    int j = 0, c0 = 0, chunks = 0;
    while (c0 < n_blocks) {
        const CsmRunChunk ch = csm_run_chunk(n_blocks, first, every, n_frames, piece, c0, j);
        const int n_new = ch.c1 - c0;
        CHECK(n_new >= 1 && n_new <= kRunChunk && ch.c1 <= n_blocks, "chunk [%d, %d) of %d", c0, ch.c1, n_blocks);
        CHECK(ch.nf >= 0 && ch.nf <= piece && j + ch.nf <= n_frames, "chunk at %d shows %d frames behind %d", c0, ch.nf, j);
        if (n_new < 1 || ch.nf < 0 || j + ch.nf > n_frames) return;  // (no endless loop)
        for (int k = 0; k < ch.nf; k++) {  // the frames in order, each in the chunk that holds its block
            const int t = first + (j + k) * every;
            CHECK(t >= c0 && t < ch.c1, "frame %d (block %d) in chunk [%d, %d)", j + k, t, c0, ch.c1);
            for (int carried_in = 0; carried_in <= keep; carried_in++) {
                const CsmRunWindow win = csm_run_window(t, keep, carried_in, c0);
                CHECK(win.n == std::min(length, t + 1 + carried_in) && win.lo == t - win.n + 1, "window of block %d: lo %d n %d", t, win.lo, win.n);
                CHECK(win.slot >= 0 && win.slot + win.n <= keep + n_new && win.slot == keep + win.lo - c0, "window of block %d in chunk [%d, %d): slot %d n %d", t, c0,
                      ch.c1, win.slot, win.n);
            }
        }
        // the next frame lies behind the chunk, unless the piece was full: then the chunk ends one block behind its last frame
        const bool more = j + ch.nf < n_frames, cut_short = ch.c1 < std::min(c0 + kRunChunk, n_blocks);
        if (more && ch.nf < piece) CHECK(first + (j + ch.nf) * every >= ch.c1, "a frame left behind in chunk [%d, %d)", c0, ch.c1);
        if (cut_short) CHECK(ch.nf == piece && ch.c1 == first + (j + ch.nf - 1) * every + 1, "chunk [%d, %d) cut short", c0, ch.c1);
        if (more && ch.nf == piece && !cut_short) CHECK(first + (j + ch.nf) * every >= ch.c1, "a full piece not cut in chunk [%d, %d)", c0, ch.c1);
        j += ch.nf, c0 = ch.c1, chunks++;
    }
    CHECK(c0 == n_blocks && j == n_frames, "%d blocks: the walk ends at %d with %d of %d frames", n_blocks, c0, j, n_frames);
    CHECK(chunks >= (n_blocks + kRunChunk - 1) / kRunChunk, "%d chunks", chunks);
}

int main() {
    check_layout();
    for (int n_blocks = 1; n_blocks <= 600; n_blocks++)
        for (int every : {1, 2, 3, 7, 300})
            for (int first : {0, 1, every - 1})
                for (int piece : {1, 2, 5})
                    for (int length : {1, 2, 3, 9}) check_walk(n_blocks, first, every, piece, length);
    for (int keep : {0, 1, 8, 1023})
        for (int carried_in = 0; carried_in <= keep; carried_in += std::max(1, keep / 5))
            for (int n_blocks : {1, 2, 7, 8, 9, 300, 2147483647})
                CHECK(csm_run_carried(carried_in, n_blocks, keep) == ((long long) carried_in + n_blocks >= keep ? keep : carried_in + n_blocks), "carried");
    CHECK(csm_run_piece(0, 8) == 1 && csm_run_piece(3, 8) == 3 && csm_run_piece(9, 8) == 8 && csm_run_piece(5, 1) == 1, "piece");
    CHECK(csm_run_chunk_blocks(1) == 1 && csm_run_chunk_blocks(256) == 256 && csm_run_chunk_blocks(300) == 256 && kRunChunk == 256 && kBlocksPerLaunch == 1024, "chunk");
    if (failures) std::printf("csm run plan: %d FAILED\n", failures);
    else std::printf("csm run plan: ok\n");
    return failures ? 1 : 0;
}
