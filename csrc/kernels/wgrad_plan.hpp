// Which kernel computes a convolution's weight gradient, on which tile, with how many split-K
// splits: the whole policy of conv_wgrad.hip's kernels, as host-only C++ (no HIP, no torch), so it
// can be compiled, run and tested without a GPU (tests/test_wgrad_plan.py).
//
//   conv_wgrad_route(shape)                        library | square family | rectangular family
//   conv_wgrad_plan(shape, family, variant, splits) kernel + its parameters, geometry and splits
//
// The two families are the two bindings: "square" = conv_wgrad (1x1 / 3x3 pad (ks-1)/2, channel
// counts % 64, ResNet / VGG / the linear layers), "rectangular" = conv_wgrad_rect (any KH x KW
// window with zero padding, channel counts % 8, Inception-v3).
#pragma once

#include <cstdint>

namespace kfk {

struct WgradShape {
    int N, H, W, Cin, Cout, kh, kw, ph, pw, stride;
    int OH() const { return (H + 2 * ph - kh) / stride + 1; }
    int OW() const { return (W + 2 * pw - kw) / stride + 1; }
    int64_t P() const { return static_cast<int64_t>(N) * OH() * OW(); }  // output pixels: the GEMM's K
    int taps() const { return kh * kw; }
};
// the square family's shape: a ks x ks window with padding (ks - 1) / 2
inline WgradShape wgrad_square_shape(int N, int H, int W, int Cin, int Cout, int ks, int stride) {
    return {N, H, W, Cin, Cout, ks, ks, (ks - 1) / 2, (ks - 1) / 2, stride};
}

// ---- the kernels' geometry arguments (conv_wgrad.hip) ---------------------------------------
// wgrad_kernel / wgrad_reduce_kernel
struct WGeo {
    int N, H, W, C, OH, OW, K;
    int P, HW;
    uint64_t m_hw, m_ow;  // floor(p / d) = (p * m) >> 40, exact for p * d < 2^40
    int mtiles, ntiles, taps, tiles, splits, kps;
    int kwin, ph, pw;  // KS == 0 (any window): taps per kernel row and the zero padding
};
// wgrad_rows_kernel
struct RGeo {
    int N, H, W, C, K;
    int L, R, spr, gpi, nseg;  // segment: L pixels per row, R rows; segments per row / per image
    int XW, xrows, xpieces;    // input image: XW = L + 2 pixels per row, xrows rows, 1 KB pieces
    int mtiles, ntiles, tiles, splits, kps;
};
// wgrad_rows_rect_kernel
struct RRGeo {
    int N, H, W, C, K, OH, OW;
    int KH, KW, ph, pw, taps, tgroups;
    int L, R, spr, gpi, nseg;
    int XW, xrows, xpieces;
    int mtiles, ntiles, tiles, splits, kps;
    int stage;  // LDS bytes per ring stage: dy | image | 1 KB dummy
    int S;      // stride (1, or 2 on the ring variants)
};

// ---- kernels, families, variant codes ---------------------------------------------------------
enum class WgradKernel {
    Tiled,     // wgrad_kernel: one workgroup per tap and wm x wn x tn tile
    Rows3x3,   // wgrad_rows_kernel<2>: 3x3 / stride 1, 64-channel tiles, 9 waves share a staged row image
    RowsRect,  // wgrad_rows_rect_kernel<7|9, 2>: any stride-1 window, 64-channel tiles, 64-pixel-row segments
    RowsRing,  // wgrad_rows_rect_kernel<7|9, stages, ct, true>: fewest-staged-rows segments, an LDS ring
               // sized to the segment, dw-layout split partials; stride 1 or 2
};
enum class WgradFamily { Square, Rect };
enum class WgradRoute { Library, Square, Rect };

// The integer variant codes of the bindings (conv_wgrad(..., variant), conv_wgrad_rect(..., variant)):
// the tuning handle of the tests and the tools.  Tile codes are co x ci channels per workgroup.
enum WgradVariant : int {
    kWgradAuto = -1,     // the planner's choice
    kWgradTile128x128 = 0,
    kWgradTile128x64 = 1,
    kWgradTile64x128 = 2,
    kWgradTile64x64 = 3,
    kWgradTile256x128 = 4,
    kWgradTile128x256 = 5,
    kWgradRows = 6,      // the row-image kernel with 64-channel tiles: Rows3x3 on the square family,
                         // RowsRect on the rectangular one
    kWgradTile256x256 = 7,  // 8 waves of 64 x 128: twice the MFMAs per staged byte
    kWgradRing32x2 = 8,  // RowsRing (rectangular family only): channel tile x ring stages
    kWgradRing32x3 = 9,
    kWgradRing32x4 = 10,
    kWgradRing64x3 = 11,
    kWgradRing64x4 = 12,
    kWgradRowsAuto = 13,  // rectangular family only: the row-image code the shape rule picks (kWgradRows or a ring code)
};
constexpr int kWgradSquareVariants = 8;  // conv_wgrad's explicit codes are 0 .. 7

const char *wgrad_kernel_name(WgradKernel k);
const char *wgrad_route_name(WgradRoute r);

struct WgradPlan {
    WgradShape shape{};          // what it was planned for
    WgradKernel kernel = WgradKernel::Tiled;
    int variant = 0;             // the resolved code (never kWgradAuto / kWgradRowsAuto)
    int wm = 0, wn = 0, tn = 0;  // Tiled: waves (co, ci) and 16-channel ci blocks per wave
    int ct = 0, stages = 0;      // row-image kernels: channel tile and LDS ring stages
    int splits = 1;              // K (pixel) splits
    int kps = 0;                 // K units (64-pixel steps or segments) per split
    int64_t ws_floats = 0;       // f32 workspace of the split partials (0: none)
    // the kernel's geometry argument, splits and kps filled in: the member `kernel` names
    WGeo tiled{};   // Tiled
    RGeo rows{};    // Rows3x3
    RRGeo rect{};   // RowsRect, RowsRing
    int bm() const { return 64 * wm; }
    int bn() const { return 16 * tn * wn; }
};

// ---- the policy ---------------------------------------------------------------------------
bool conv_wgrad_supported(int Cin, int Cout, int ks, int stride);                   // square family
bool conv_wgrad_rect_supported(int Cin, int Cout, int kh, int kw, int stride);      // rectangular family
bool conv_wgrad_rows_rect_supported(const WgradShape &s);  // a row-image kernel of the rectangular family covers it
// what kWgradRowsAuto resolves to (kWgradRows or a ring code); the shape must be rows_rect_supported
int conv_wgrad_rows_rect_auto(const WgradShape &s);

// variant: a code of `family`, or kWgradAuto; splits: -1 = the planner's (the square family only takes
// an explicit count).  Throws std::invalid_argument for a code the shape or the family does not allow.
WgradPlan conv_wgrad_plan(const WgradShape &s, WgradFamily family, int variant = kWgradAuto, int splits = -1);

struct WgradRouting {
    WgradRoute route;
    int variant;         // resolved code to pass to the family's binding (kWgradAuto for Library)
    int64_t max_pixels;  // output pixels (N*OH*OW) one launch of that plan handles
};
// Which family takes this convolution's weight gradient, or the library (MIOpen).
WgradRouting conv_wgrad_route(const WgradShape &s);

// ---- shared launch arithmetic ---------------------------------------------------------------
// wgrad_reduce_kernel's launch for `total4` float4 outputs summed over `splits` partials
struct WgradReduceLaunch {
    int sg_log2;  // split groups per block (log2): enough blocks for the chip, at most 64 groups, <= splits
    int grid;
};
WgradReduceLaunch wgrad_reduce_launch(int64_t total4, int splits);

}  // namespace kfk
