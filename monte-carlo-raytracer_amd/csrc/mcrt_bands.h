// mcrt_bands.h -- the arithmetic of a band split: an image of H rows is cut into 8-row blocks, and
// bands of bandRows rows (bandRows / 8 blocks) are dealt to the numBands ranks in turn, so block gb
// belongs to rank (gb / (bandRows / 8)) % numBands.  Host only, no HIP header.
#pragma once
#include <algorithm>
#include <cstdint>

namespace mcrt {

// 8-row blocks of rank r: the whole deals' share plus what the last, partial deal leaves for r
inline int band_blocks(uint32_t H, int bandRows, int numBands, int r) {
    const int blocks = (int)((H + 7) / 8), bpb = bandRows / 8;
    const int perDeal = bpb * numBands;
    return (blocks / perDeal) * bpb + std::min(std::max(blocks % perDeal - r * bpb, 0), bpb);
}

// The largest rank's row count (whole blocks; rank 0 is dealt first, so it holds the most): the
// rows of one chunk of the packed accumulator exchange and of the rank-major splat layout.
inline int band_max_rows(uint32_t H, int bandRows, int numBands) { return 8 * band_blocks(H, bandRows, numBands, 0); }

}  // namespace mcrt
