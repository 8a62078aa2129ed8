// image_loss.hpp -- geometry and state layout of the fused photometric loss (image_loss.hip), shared by the
// kernels, the entries of api.hip and -- the tile constants -- the tests, which read them from this file.
#pragma once
#include "common.hpp"

namespace gsr {

constexpr int IL_TILE_W = 32;   // loss pixels per workgroup tile, x
constexpr int IL_TILE_H = 32;   // ... and y
constexpr int IL_HALO = 5;      // the 11-tap window reaches 5 pixels past the tile on every side
constexpr int IL_THREADS = 256; // both tile kernels and the sum kernel
constexpr int IL_SUMS = 3;      // per-tile partial sums: |x - y|, m, (x - y)^2

// The caller's state block, behind align256 of its pointer:
//   partials [V][il_parts(W, H)][IL_SUMS] double   the partial sums of every (tile, channel), in tile-major order
//   maps     [V][3 maps A B C][3 channels][H][W] float
struct ImageLossState {
    double* partials;
    float* maps;
    size_t bytes;   // what gsr_image_loss_state_bytes returns: both arrays and 256 B for aligning the caller's pointer
};
inline int64_t il_parts(int W, int H) { return div_up(W, IL_TILE_W) * div_up(H, IL_TILE_H) * 3; }
inline ImageLossState image_loss_state(void* base, int V, int W, int H)
{
    ImageLossState s;
    char* cur = reinterpret_cast<char*>(base);
    carve(cur, s.partials, (size_t)V * (size_t)il_parts(W, H) * IL_SUMS);
    carve(cur, s.maps, (size_t)V * 9 * (size_t)W * (size_t)H);
    s.bytes = (size_t)(cur - reinterpret_cast<char*>(base)) + 256;
    return s;
}

}  // namespace gsr
