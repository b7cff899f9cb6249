// The tile plan of a label map at one level (spade_tiles.hip writes it, spade_fused.hip reads it): which 16x16-pixel tiles of
// patch_tiles(N, H, W) carry ONE one-hot label over their whole 20x20 patch ("light": gamma|beta are one of <= 8 constant vectors)
// and which need the matrix work ("heavy").  int32 words, m = patch_tiles(N, H, W):
//     [ST_NHEAVY] [ST_NLIGHT]                 the two counts (they add up to m)
//     [ST_REP + k], k = 0..7                  the representative of class k: the lowest light-classified tile of that class, or -1.
//                                             It is on the HEAVY list, flagged, and fills row k of the launch's gamma|beta table
//     [ST_HDR, ST_HDR + m)                    heavy list, ascending tile number: tile | (k + 1) << 24 for a representative
//     [ST_HDR + m, ST_HDR + 2 m)              light list, ascending tile number: tile | k << 24
//     [ST_HDR + 2 m, ST_HDR + 3 m)            scratch: the class of every tile (-1 heavy)
#pragma once

namespace hrv {
constexpr int ST_NHEAVY = 0, ST_NLIGHT = 1, ST_REP = 2, ST_HDR = 16;
constexpr int ST_TILE_MASK = 0xFFFFFF;
constexpr long long ST_MAX_TILES = 1 << 24;
}  // namespace hrv
