// Host check of rodeo_amd/csrc/tile3_pack.hpp (built and run by tests/test_tile3_pack_host.py): the invariants the header
// states, exhaustively for every N in 16 .. 300, all four tiles of a tile-wave and all nine slots of a record.
#include <cstdio>
#include <vector>

#include "tile3_pack.hpp"

using namespace rk;

static int fails = 0;
#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            if (++fails <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                            \
    } while (0)

constexpr int CHUNK = 16, ZONE_BYTES = 6144;

int main() {
    // the slots: upper triangle row-major, then the mean column; a bijection onto 0 .. 8; nothing for the lower triangle
    {
        int seen[9] = {0};
        const int want[3][4] = {{0, 1, 2, 6}, {-1, 3, 4, 7}, {-1, -1, 5, 8}};
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) {
                const int s = tile3_pack_slot(r, c);
                CHECK(s == want[r][c], "slot(%d,%d) = %d", r, c, s);
                if (s >= 0 && s < 9) ++seen[s];
            }
        for (int s = 0; s < 9; ++s) CHECK(seen[s] == 1, "slot %d used %d times", s, seen[s]);
    }
    CHECK(tile3_pack_full_wave(0, 4) && !tile3_pack_full_wave(0, 3) && tile3_pack_full_wave(1, 8) && !tile3_pack_full_wave(1, 7) &&
              !tile3_pack_full_wave(2, 10), "full_wave");

    long records = 0;
    for (int N = T3P_MIN_STEPS; N <= 300; ++N) {
        // ---- invariants 1 and 2: the forward kernel packs the steps 0 .. N-1 ----
        std::vector<int> owner((size_t)(N + 1) * T3P_STRIPE, -1);      // byte of the tile-wave's stripe rows 0 .. N -> step
        for (int n = 0; n < N; ++n)
            for (int g = 0; g < 4; ++g)
                for (int slot = 0; slot < 9; ++slot) {
                    const int gb = tile3_pack_group_byte(n, g, slot);
                    const int row = tile3_pack_row(n >> 2, gb), col = tile3_pack_col(gb);
                    CHECK(gb >= 0 && gb + 8 <= T3P_GROUP, "N %d n %d g %d slot %d: group byte %d", N, n, g, slot, gb);
                    CHECK(col % 8 == 0 && col + 8 <= T3P_STRIPE, "N %d n %d: col %d leaves the stripe", N, n, col);
                    CHECK(row >= 1 && row <= N - 1, "N %d n %d g %d slot %d: row %d outside 1 .. N-1", N, n, g, slot, row);
                    CHECK(n >= row - 1, "N %d: row %d holds step %d", N, row, n);
                    // what the forward kernel computes: the offset inside group 0 plus three rows per group
                    CHECK(row == 3 * (n >> 2) + tile3_pack_row(0, gb), "N %d n %d: row %d is not group-relative", N, n, row);
                    if (row < 0 || row > N) continue;
                    for (int b = 0; b < 8; ++b) {
                        int& o = owner[(size_t)row * T3P_STRIPE + col + b];
                        CHECK(o == -1, "N %d: byte (%d, %d) of steps %d and %d", N, row, col + b, o, n);
                        o = n;
                    }
                    ++records;
                }
        for (int col = 0; col < T3P_STRIPE; ++col)
            CHECK(owner[col] == -1 && owner[(size_t)N * T3P_STRIPE + col] == -1, "N %d: row 0 or N touched", N);

        // ---- invariant 3: the smoother's chunks (steps N-1 .. 1, 16 per chunk from the top) ----
        const int n_chunks = (N - 1 + CHUNK - 1) / CHUNK;
        std::vector<char> handed(N, 0);
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int n_hi = N - 1 - ch * CHUNK;
            const int n_lo = N - CHUNK - ch * CHUNK < 1 ? 1 : N - CHUNK - ch * CHUNK;
            const int first = tile3_pack_chunk_first_row(n_lo), rows = tile3_pack_chunk_rows(n_lo, n_hi);
            CHECK(rows >= 3 && rows <= 15 && rows * T3P_STRIPE <= ZONE_BYTES, "N %d chunk %d: %d stripe rows", N, ch, rows);
            if (n_hi - n_lo == CHUNK - 1 && n_hi % 4 == 3) CHECK(rows == 12, "N %d chunk %d: %d rows, not 12", N, ch, rows);
            CHECK(first >= 1 && first + rows - 1 <= N - 1, "N %d chunk %d: rows %d .. %d", N, ch, first, first + rows - 1);
            std::vector<int> zone_owner((size_t)rows * T3P_STRIPE, -1);
            for (int n = n_lo; n <= n_hi; ++n) {
                CHECK(!handed[n], "N %d: step %d in two chunks", N, n);
                handed[n] = 1;
                for (int g = 0; g < 4; ++g)
                    for (int slot = 0; slot < 9; ++slot) {
                        const int zb = tile3_pack_zone_byte(n_lo, n, g) + 8 * slot;
                        CHECK(zb >= 0 && zb + 8 <= rows * T3P_STRIPE, "N %d chunk %d n %d: zone byte %d", N, ch, n, zb);
                        if (zb < 0 || zb + 8 > rows * T3P_STRIPE) continue;
                        CHECK(zone_owner[zb] == -1, "N %d chunk %d: zone byte %d twice", N, ch, zb);
                        zone_owner[zb] = n;
                        // the 16-byte piece that brings this zone byte in, and where it comes from
                        const int j = zb / 16, src_row = first + j / 24, src_col = (j % 24) * 16 + zb % 16;
                        const int gb = tile3_pack_group_byte(n, g, slot);
                        CHECK(src_row == tile3_pack_row(n >> 2, gb) && src_col == tile3_pack_col(gb),
                              "N %d chunk %d n %d g %d slot %d: piece reads (%d, %d), record is at (%d, %d)", N, ch, n, g, slot,
                              src_row, src_col, tile3_pack_row(n >> 2, gb), tile3_pack_col(gb));
                        CHECK(owner[(size_t)src_row * T3P_STRIPE + src_col] == n, "N %d n %d: piece reads another step", N, n);
                    }
            }
        }
        for (int n = 1; n < N; ++n) CHECK(handed[n], "N %d: step %d in no chunk", N, n);
    }
    std::printf("%ld records checked, %d failure(s)\n", records, fails);
    return fails ? 1 : 0;
}
