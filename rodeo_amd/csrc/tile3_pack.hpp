// Packed in-place layout of the p = 3 filtered rows between fwd_tile3_kernel and bwd_mv_tile3_kernel (solve_mv only).
// Plain constexpr functions, no HIP headers: the kernels, hiprtc and a host program (tests/test_tile3_pack_host.py) read
// the same map.  With RK_FLAG_TILE3_PACKED_MV the smoother leaves its SMOOTHED rows in the same records (RK_LAYOUT_TILE3_PACKED
// of include/rodeo_kalman.h): the record of step n over the filtered record of step n, so invariant 1 covers them as it stands,
// and the readers of such an array (records.hpp, gauss_logpost_kernel, SolvePlan on the host through rk_tile3_packed_waves;
// tests/test_tile3_pack_out_host.py) use the predicates at the end of this header.
//
// The smoother reads every filtered tile [Sigma_f | mu_f] once, 96 B of which 24 are the lower triangle of a symmetric
// matrix.  A packed record is the upper triangle row-major, then mu_f: 9 doubles = 72 B.  It lives INSIDE the tile array:
//   stripe     bytes [384 tw, 384 tw + 384) of a time row: the four tiles of tile-wave tw (one forward wave, one
//              backward workgroup); only FULL tile-waves pack (a ragged last one has a narrower stripe and stays natural)
//   group k    the records of steps 4 k .. 4 k + 3 of the tile-wave, 4 x 4 x 72 = 1152 B = three stripes, stored
//              contiguously (step-major, then tile) over the stripe rows 3 k + 1, 3 k + 2, 3 k + 3
// Rows 0 and N keep the natural 96-byte tiles.  Invariants (checked exhaustively by the host program):
//   1. (step, tile-in-wave, slot) -> (stripe row, byte) is injective and stays in the stripe rows 1 .. N - 1 of the
//      tile-wave's own stripe: never row 0, row N or the scratch tail, never another tile-wave's bytes.
//   2. Stripe row m holds bytes of steps n >= m - 1 only.  The smoother's chain (natural output) writes the smoothed natural row m over
//      its own stripe when it reaches step m, i.e. after every step > m; step m - 1 is at most one chunk ahead and was
//      fetched at least two ticks earlier (bwd_mv_tile3_kernel).  So a workgroup only overwrites records it has consumed.
//   3. A chunk's records are whole groups, i.e. whole 384-byte stripes in 16-byte pieces (lds_dma16): the 16 steps
//      n_hi - 15 .. n_hi touch 5 groups = 15 stripes, 4 groups = 12 stripes when n_hi % 4 == 3.
#pragma once

namespace rk {

constexpr int T3P_STRIPE = 384;                 // four natural tiles
constexpr int T3P_REC = 72;                     // packed record of one tile
constexpr int T3P_STEP = 4 * T3P_REC;           // one step of a tile-wave
constexpr int T3P_GROUP = 4 * T3P_STEP;         // four steps = three stripes
constexpr int T3P_MIN_STEPS = 16;               // below: natural (the first group's rows 1 .. 3 must lie below row N)
static_assert(T3P_GROUP == 3 * T3P_STRIPE, "four packed steps are three stripes");

// a tile-wave packs only if all four of its tiles exist
constexpr bool tile3_pack_full_wave(int tw, int n_tiles) { return 4 * tw + 4 <= n_tiles; }

// slot (0..8) of element (r, c) of the 3 x 4 tile [Sigma | mu] in the packed record, -1 for the lower triangle
constexpr int tile3_pack_slot(int r, int c) {
    return c == 3 ? 6 + r : (c < r ? -1 : (r == 0 ? c : (r == 1 ? 2 + c : 5)));
}
// byte of (step n, tile g, slot) inside its group
constexpr int tile3_pack_group_byte(int n, int g, int slot) { return (n & 3) * T3P_STEP + g * T3P_REC + slot * 8; }
// stripe row and byte inside the stripe of byte `gb` of group k
constexpr int tile3_pack_row(int k, int gb) { return 3 * k + 1 + gb / T3P_STRIPE; }
constexpr int tile3_pack_col(int gb) { return gb % T3P_STRIPE; }

// The smoother's chunk of the steps n_lo .. n_hi (n_lo >= 1): its groups, the stripe rows they occupy (first row and
// count; piece j of 16 bytes is bytes 16 (j % 24) of stripe row first + j / 24 and lands at byte 16 j of the zone),
// and where step n's record of tile g then starts in the zone.
constexpr int tile3_pack_chunk_first_row(int n_lo) { return 3 * (n_lo >> 2) + 1; }
constexpr int tile3_pack_chunk_rows(int n_lo, int n_hi) { return 3 * ((n_hi >> 2) - (n_lo >> 2) + 1); }
constexpr int tile3_pack_zone_byte(int n_lo, int n, int g) {
    return ((n >> 2) - (n_lo >> 2)) * T3P_GROUP + (n & 3) * T3P_STEP + g * T3P_REC;
}

// ---- where records are packed: the ONE rule of the forward kernel's stores, the smoother's reads and stores, and every
// reader of a packed array (records.hpp, rk_tile3_packed_waves for the host) ----
// The sizes at which solve_mv packs at all: the first group's rows 1 .. 3 below row N, and the whole tile array inside one
// store window of the forward kernel.
constexpr long long T3P_MAX_BYTES = 0x7fff0000ll;
constexpr bool tile3_pack_sizes(long long n_steps, long long n_tiles) {
    return n_steps >= T3P_MIN_STEPS && (n_steps + 1) * n_tiles * 96 < T3P_MAX_BYTES;
}
// tile-waves whose steps 1 .. N - 1 are packed records: the full ones, at those sizes
constexpr int tile3_pack_waves(long long n_steps, long long n_tiles) {
    return tile3_pack_sizes(n_steps, n_tiles) ? (int)(n_tiles / 4) : 0;
}
// is the record of (step n, tile tau) a packed one?  Rows 0 and N and ragged tile-waves stay natural.
constexpr bool tile3_pack_record(long long n_steps, long long n_tiles, long long n, long long tau) {
    return n >= 1 && n < n_steps && tau < 4ll * tile3_pack_waves(n_steps, n_tiles);
}
// index (in doubles, from the start of the tile array) of the packed record of (step n, tile tau), and of its slot: a record
// is 9 doubles, contiguous but for the step from one stripe row to the next (72 does not divide 384)
constexpr long long tile3_pack_index(long long n_tiles, long long n, long long tau, int slot) {
    const int gb = tile3_pack_group_byte((int)(n & 3), (int)(tau & 3), slot);
    return (long long)tile3_pack_row((int)(n >> 2), gb) * n_tiles * 12 + (tau >> 2) * (T3P_STRIPE / 8) + tile3_pack_col(gb) / 8;
}

}  // namespace rk
