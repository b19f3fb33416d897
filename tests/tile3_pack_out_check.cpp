// Host check of the packed SMOOTHED rows of solve_mv at p = 3 (RK_LAYOUT_TILE3_PACKED): includes the header the kernels
// include (rodeo_amd/csrc/tile3_pack.hpp) and sweeps every (N <= 70, tile count <= 12, step, tile, slot).
//   * the record predicate: packed exactly for the steps 1 .. N-1 of the tiles of full tile-waves, at N >= 16
//   * tile3_pack_index is injective, stays out of the rows 0 and N and inside the tile-wave's own stripe, and is the byte of
//     the FILTERED record as the issue words it: group n >> 2, stripe rows 3k+1 .. 3k+3, byte (n & 3) 288 + 72 g + 8 slot
//   * the smoother's store offsets (per-lane byte by n & 3, scalar row by step-in-chunk, chunk base row) reach that byte
// argv[1]: a file that receives, per (N, tiles) in sweep order, the int32 words [N, tiles, W] followed -- where W > 0 -- by
// tile3_pack_index for (step 1 .. N-1, tile 0 .. 4W-1, slot 0 .. 8): what tests/test_tile3_pack_out_host.py holds the Python
// gathers against.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "tile3_pack.hpp"

using namespace rk;

static long failures = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            if (failures < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
            ++failures;                                       \
        }                                                     \
    } while (0)

int main(int argc, char** argv) {
    std::FILE* out = argc > 1 ? std::fopen(argv[1], "wb") : nullptr;
    if (argc > 1 && !out) { std::printf("cannot open %s\n", argv[1]); return 2; }
    constexpr int CHUNK = 16;
    long records = 0;
    for (int N = 1; N <= 70; ++N)
        for (int T = 1; T <= 12; ++T) {
            const int W = tile3_pack_waves(N, T);
            CHECK(W == (N >= 16 ? T / 4 : 0), "N %d T %d W %d", N, T, W);
            const int32_t head[3] = {N, T, W};
            if (out) std::fwrite(head, sizeof(int32_t), 3, out);
            const long long row_doubles = 12ll * T;
            std::vector<int> owner((size_t)(N + 1) * row_doubles, -1);
            std::vector<int32_t> idx;
            for (int n = 0; n <= N; ++n)
                for (int tau = 0; tau < T; ++tau) {
                    const bool packed = tile3_pack_record(N, T, n, tau);
                    const bool want = N >= 16 && n >= 1 && n < N && tile3_pack_full_wave(tau >> 2, T);
                    CHECK(packed == want, "N %d T %d n %d tau %d", N, T, n, tau);
                    if (!packed) continue;
                    ++records;
                    const int tw = tau >> 2, g = tau & 3, k = n >> 2;
                    for (int slot = 0; slot < 9; ++slot) {
                        const long long i = tile3_pack_index(T, n, tau, slot);
                        const long long row = i / row_doubles, col = i % row_doubles;
                        CHECK(row >= 1 && row < N, "row %lld of N %d (n %d)", row, N, n);
                        CHECK(col >= 48ll * tw && col < 48ll * tw + 48, "col %lld outside the stripe of tile-wave %d", col, tw);
                        // the filtered record's byte, spelled out
                        const int gb = (n & 3) * 288 + g * 72 + slot * 8;
                        const long long byte = (3ll * k + 1 + gb / 384) * row_doubles * 8 + 384ll * tw + gb % 384;
                        CHECK(i * 8 == byte, "N %d T %d n %d tau %d slot %d: %lld != %lld", N, T, n, tau, slot, i * 8, byte);
                        CHECK(byte == ((long long)tile3_pack_row(k, tile3_pack_group_byte(n, g, slot)) * row_doubles * 8 + 384ll * tw +
                                       tile3_pack_col(tile3_pack_group_byte(n, g, slot))), "forward kernel's byte");
                        if (i >= 0 && i < (long long)owner.size()) {
                            CHECK(owner[(size_t)i] < 0, "N %d T %d: double %lld written twice", N, T, i);
                            owner[(size_t)i] = n;
                        }
                        idx.push_back((int32_t)i);
                        // the smoother's store: chunk t holds the steps n_hi .. n_hi - 15 with n_hi = N - 1 - 16 t; a full
                        // chunk stores step s at  base row + scalar row offset(s) + per-lane byte(s & 3)
                        const int t = (N - 1 - n) / CHUNK, n_hi = N - 1 - t * CHUNK, s = n_hi - n, ph0 = (N - 1) & 3;
                        if (n_hi >= CHUNK) {
                            const int row_lo = tile3_pack_chunk_first_row(n_hi - (CHUNK - 1));
                            const int srow = 3 * (((ph0 - s) >> 2) - ((ph0 - (CHUNK - 1)) >> 2));
                            const int ph = (ph0 - (s & 3)) & 3;
                            const int pgb = tile3_pack_group_byte(ph, g, slot);
                            const long long lane = (long long)(pgb / T3P_STRIPE) * row_doubles * 8 + pgb % T3P_STRIPE;
                            CHECK(ph == (n & 3), "phase of step %d in chunk %d", n, t);
                            CHECK(srow >= 0 && srow + pgb / T3P_STRIPE <= 14, "window of 15 rows, srow %d", srow);
                            CHECK((row_lo + srow) * row_doubles * 8 + lane + 384ll * tw == byte, "store of N %d n %d slot %d", N, n, slot);
                        }
                    }
                }
            if (out && !idx.empty()) std::fwrite(idx.data(), sizeof(int32_t), idx.size(), out);
        }
    if (out) std::fclose(out);
    std::printf("%ld packed records checked, %ld failure(s)\n", records, failures);
    return failures ? 1 : 0;
}
