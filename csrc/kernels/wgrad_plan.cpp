// The weight-gradient policy (wgrad_plan.hpp): host-only, plain C++17.
#include "wgrad_plan.hpp"

#include <algorithm>
#include <stdexcept>

namespace kfk {

namespace {

constexpr int kBK = 64;  // pixels per K-step of the tap-tiled kernel
constexpr int64_t kTiledMaxPixels = int64_t(1) << 23;  // its 40-bit magic division
constexpr int64_t kRowsMaxPixels = int64_t(1) << 31;   // row-image kernels: 32-bit element offsets only

// variant code -> kernel and parameters, indexed by the code.  Tiles: wm x wn waves of 64 co x 16 tn ci.
struct Variant {
    WgradKernel kernel;
    int wm, wn, tn;
    int ct, stages;
};
constexpr Variant kVariants[] = {
    /* kWgradTile128x128 */ {WgradKernel::Tiled, 2, 2, 4, 0, 0},
    /* kWgradTile128x64  */ {WgradKernel::Tiled, 2, 1, 4, 0, 0},
    /* kWgradTile64x128  */ {WgradKernel::Tiled, 1, 2, 4, 0, 0},
    /* kWgradTile64x64   */ {WgradKernel::Tiled, 1, 1, 4, 0, 0},
    /* kWgradTile256x128 */ {WgradKernel::Tiled, 4, 2, 4, 0, 0},
    /* kWgradTile128x256 */ {WgradKernel::Tiled, 2, 4, 4, 0, 0},
    /* kWgradRows        */ {WgradKernel::Rows3x3, 0, 0, 0, 64, 2},  // RowsRect on the rectangular family
    /* kWgradTile256x256 */ {WgradKernel::Tiled, 4, 2, 8, 0, 0},
    /* kWgradRing32x2    */ {WgradKernel::RowsRing, 0, 0, 0, 32, 2},
    /* kWgradRing32x3    */ {WgradKernel::RowsRing, 0, 0, 0, 32, 3},
    /* kWgradRing32x4    */ {WgradKernel::RowsRing, 0, 0, 0, 32, 4},
    /* kWgradRing64x3    */ {WgradKernel::RowsRing, 0, 0, 0, 64, 3},
    /* kWgradRing64x4    */ {WgradKernel::RowsRing, 0, 0, 0, 64, 4},
};
static_assert(sizeof(kVariants) / sizeof(kVariants[0]) == kWgradRing64x4 + 1, "one row per code");

WgradPlan plan_of(WgradFamily family, int variant) {
    const Variant &v = kVariants[variant];
    WgradPlan pl;
    pl.kernel = variant == kWgradRows && family == WgradFamily::Rect ? WgradKernel::RowsRect : v.kernel;
    pl.variant = variant;
    pl.wm = v.wm, pl.wn = v.wn, pl.tn = v.tn, pl.ct = v.ct, pl.stages = v.stages;
    return pl;
}

// `want` splits over `units` K units, at least `min_units` per split (but one split always), no empty split
void split_k(WgradPlan &pl, int units, int want, int min_units) {
    const int splits = std::max(1, std::min(want, std::max(1, units / min_units)));
    pl.kps = (units + splits - 1) / splits;
    pl.splits = (units + pl.kps - 1) / pl.kps;
}

uint64_t magic40(int d) { return (uint64_t(1) << 40) / static_cast<uint64_t>(d) + 1; }

// ---- geometry builders -----------------------------------------------------------------------

// channel counts that are not multiples of the tile: the last tile is zero-padded (rectangular family)
WGeo tiled_geo(const WgradShape &s, const WgradPlan &pl) {
    WGeo g{};
    g.N = s.N, g.H = s.H, g.W = s.W, g.C = s.Cin, g.K = s.Cout;
    g.OH = s.OH(), g.OW = s.OW();
    g.HW = g.OH * g.OW;
    g.P = static_cast<int>(s.P());
    g.m_hw = magic40(g.HW);
    g.m_ow = magic40(g.OW);
    g.mtiles = (s.Cout + pl.bm() - 1) / pl.bm();
    g.ntiles = (s.Cin + pl.bn() - 1) / pl.bn();
    g.taps = s.taps();
    g.tiles = g.mtiles * g.ntiles * g.taps;
    g.kwin = s.kw, g.ph = s.ph, g.pw = s.pw;
    return g;
}

// 3x3 / pad 1 / stride 1, channel counts % 64: segments of 64 consecutive pixels of an output row
// (W >= 64) or 64 / W whole rows
RGeo rows3x3_geo(const WgradShape &s) {
    RGeo g{};
    g.N = s.N, g.H = s.H, g.W = s.W, g.C = s.Cin, g.K = s.Cout;
    if (s.W >= 64) {
        g.L = 64, g.R = 1, g.spr = (s.W + 63) / 64, g.gpi = s.H;
    } else {
        g.L = s.W, g.R = 64 / s.W, g.spr = 1, g.gpi = (s.H + g.R - 1) / g.R;
    }
    g.nseg = s.N * g.gpi * g.spr;
    g.XW = g.L + 2;
    g.xrows = (g.R + 2) * g.XW;
    g.xpieces = (g.xrows + 7) / 8;
    g.mtiles = s.Cout / 64, g.ntiles = s.Cin / 64;
    g.tiles = g.mtiles * g.ntiles * 9;
    return g;
}

// How wgrad_rows_rect_kernel's segment of 64 output pixels is shaped
enum class RowSegments {
    PixelRow,     // as rows3x3_geo (64 pixels of a row, or 64 / OW whole rows); a fixed 25 KB image stage
    FewestStaged  // the R x L shape with the fewest staged rows (dy + image); a stage sized to the segment
};

// the row-image kernel's segments / tap groups for a KH x KW window (xpieces > 25: unsupported)
RRGeo rows_rect_geo(const WgradShape &s, int ct, RowSegments seg) {
    RRGeo g{};
    const int stride = s.stride;
    g.N = s.N, g.H = s.H, g.W = s.W, g.C = s.Cin, g.K = s.Cout, g.S = stride;
    g.OH = s.OH(), g.OW = s.OW();
    g.KH = s.kh, g.KW = s.kw, g.ph = s.ph, g.pw = s.pw, g.taps = s.taps();
    const int nwv = g.taps % 7 == 0 ? 7 : 9;
    g.tgroups = (g.taps + nwv - 1) / nwv;
    auto shape = [&](int L, int R) {
        g.L = L, g.R = R, g.spr = (g.OW + L - 1) / L, g.gpi = (g.OH + R - 1) / R;
        g.nseg = s.N * g.gpi * g.spr;
        g.XW = stride * (g.L - 1) + s.kw;
        g.xrows = (stride * (g.R - 1) + s.kh) * g.XW;
    };
    if (seg == RowSegments::PixelRow) {
        if (g.OW >= 64) shape(64, 1);
        else shape(g.OW, 64 / g.OW);
    } else {
        // 64-byte rows: the R x L segment of 64 slots with the fewest staged rows (dy + image) in
        // total -- R > 1 on the wide maps too (Conv2d_2a's 109-wide rows: 16 x 4 stages 1.7 input
        // rows per output pixel where 64 x 1 stages 3.1)
        int64_t best = -1;
        int bl = 64, br = 1;
        for (int R = 1; R <= 64; ++R) {
            const int L = std::min(g.OW, 64 / R);
            if (L < 1 || (R > 1 && (R - 1) * L >= 64)) break;
            if (R > g.OH + 1) break;
            shape(L, R);
            if (g.xrows * 2 * ct > 25 * 1024) continue;
            const int64_t cost = static_cast<int64_t>(g.nseg) * (64 + g.xrows);
            if (best < 0 || cost < best) best = cost, bl = L, br = R;
        }
        shape(bl, br);
    }
    g.xpieces = (g.xrows * 2 * ct + 1023) / 1024;
    g.mtiles = (s.Cout + ct - 1) / ct, g.ntiles = (s.Cin + ct - 1) / ct;
    g.stage = 64 * 2 * ct + (seg == RowSegments::PixelRow ? 26 : g.xpieces + 1) * 1024;
    g.tiles = g.mtiles * g.ntiles * g.taps;
    return g;
}

// ---- the square family (conv_wgrad) ----------------------------------------------------------

bool rows3x3_supported(const WgradShape &s) {
    return s.kh == 3 && s.stride == 1 && s.Cin % 64 == 0 && s.Cout % 64 == 0;
}

int square_default(const WgradShape &s) {
    const int Cin = s.Cin, Cout = s.Cout;
    // every stride-1 3x3 (tools/bench_wgrad.py, profiles/r6_wgrad_plan.md: ResNet-50's 14 x 14 256->256 and
    // 7 x 7 512->512 113 -> 93 us against the tiles, VGG-16's 56 x 56 128->256 / 256->256 673 -> 766 /
    // 688 -> 788 TF/s)
    if (rows3x3_supported(s)) return kWgradRows;
    // tools/bench_wgrad.py --sweep (profiles/README.md): 8-wave 256x128 tiles once the GEMM is big
    // enough, else the largest 4/2/1-wave tile the channel counts allow.
    // tools/bench_wgrad_1x1.py: 256x256 for the large long-K linear-layer products (BERT-base 768x3072
    // at 16 K tokens: 133 -> 87 us) and the wide 1x1 products on >= 200,704 output pixels (28 x 28
    // 512->256 103 -> 77 us, 56 x 56 256->512 / s2 103 -> 90); ResNet's other 1x1 shapes keep 256x128
    // (their split-K partials of 256x256 tiles cost more than the extra MFMA density saves)
    const int64_t work = static_cast<int64_t>(Cin) * Cout * s.taps();
    if (Cout % 256 == 0 && Cin % 256 == 0 && s.kh == 1 && (work >= 1500000 || s.P() >= 200704)) return kWgradTile256x256;
    if (Cout % 256 == 0 && Cin % 128 == 0) return kWgradTile256x128;
    // 128x256 wherever it divides (56 x 56 256->128 158 -> 111 us, 28 x 28 512->128 73 -> 60)
    if (Cout % 128 == 0 && Cin % 256 == 0) return kWgradTile128x256;
    if (Cout % 128 == 0 && Cin % 128 == 0) return kWgradTile128x128;
    if (Cout % 128 == 0) return kWgradTile128x64;
    if (Cin % 128 == 0) return kWgradTile64x128;
    return kWgradTile64x64;
}

WgradPlan plan_square(const WgradShape &s, int variant, int splits) {
    if (!conv_wgrad_supported(s.Cin, s.Cout, s.kh, s.stride)) throw std::invalid_argument("conv_wgrad: unsupported shape");
    if (variant < 0) variant = square_default(s);
    if (variant >= kWgradSquareVariants) throw std::invalid_argument("conv_wgrad: unknown variant");
    WgradPlan pl = plan_of(WgradFamily::Square, variant);
    if (pl.kernel == WgradKernel::Rows3x3) {
        if (!rows3x3_supported(s)) throw std::invalid_argument("conv_wgrad: rows variant needs 3x3/s1");
        RGeo &g = pl.rows = rows3x3_geo(s);
        if (g.xpieces > 25) throw std::invalid_argument("conv_wgrad rows: input image exceeds the stage");
        const int ct = g.mtiles * g.ntiles;
        // one workgroup of 9 waves per CU, >= 4 segments per split (two per CU doubled the split partials
        // to reduce: 56 x 56 64->64 119 -> 89 us, 28 x 28 128->128 108 -> 84)
        if (splits < 0) splits = std::max(1, (256 + ct / 2) / ct);
        split_k(pl, g.nseg, splits, 4);
        g.splits = pl.splits, g.kps = pl.kps;
        pl.ws_floats = pl.splits > 1 ? static_cast<int64_t>(pl.splits) * ct * 9 * 4096 : 0;
        return pl;
    }
    if (s.Cout % pl.bm() != 0 || s.Cin % pl.bn() != 0) throw std::invalid_argument("conv_wgrad: tile/channel mismatch");
    WGeo &g = pl.tiled = tiled_geo(s, pl);
    const int64_t P = s.P();
    const int ksteps = static_cast<int>((P + kBK - 1) / kBK);
    if (splits < 0) {
        // workgroups per launch: one per CU for the 4/8-wave tiles (2 for 3x3), more for the
        // 1-2 wave tiles, so every CU keeps >= ~48 KB of loads in flight; >= 4 K-steps per split
        const int nw = pl.wm * pl.wn;
        int target = 256 * (nw >= 4 ? 1 : 2);
        if (s.kh == 3) target *= nw == 1 ? 4 : 2;
        splits = (target + g.tiles / 2) / g.tiles;
        // large-pixel 3x3 shapes: ~100 K-steps per split and up to 512 splits (tools/bench_vgg_wgrad.py)
        if (s.kh == 3 && P >= 800000) splits = std::max(splits, std::min(512, ksteps / 96));
        split_k(pl, ksteps, splits, 4);
    } else {
        split_k(pl, ksteps, splits, 1);
    }
    g.splits = pl.splits, g.kps = pl.kps;
    pl.ws_floats = pl.splits > 1 ? static_cast<int64_t>(pl.splits) * g.tiles * pl.bm() * pl.bn() : 0;
    return pl;
}

// ---- the rectangular family (conv_wgrad_rect) -------------------------------------------------

// tile: 128 rows where the channel count reaches it (less zero padding otherwise)
int rect_tile(const WgradShape &s) {
    return s.Cout >= 128 ? (s.Cin >= 128 ? kWgradTile128x128 : kWgradTile128x64)
                         : (s.Cin >= 128 ? kWgradTile64x128 : kWgradTile64x64);
}

WgradPlan plan_rect(const WgradShape &s, int variant) {
    if (!conv_wgrad_rect_supported(s.Cin, s.Cout, s.kh, s.kw, s.stride)) throw std::invalid_argument("conv_wgrad_rect: unsupported");
    const char *no_rows = "conv_wgrad_rect: row-image variant unsupported for this shape";
    if (variant == kWgradRowsAuto) {
        if (!conv_wgrad_rows_rect_supported(s)) throw std::invalid_argument(no_rows);
        variant = conv_wgrad_rows_rect_auto(s);
    }
    if (variant >= kWgradRing32x2 && variant <= kWgradRing64x4) {
        if (!conv_wgrad_rows_rect_supported(s)) throw std::invalid_argument(no_rows);
        WgradPlan pl = plan_of(WgradFamily::Rect, variant);
        RRGeo &g = pl.rect = rows_rect_geo(s, pl.ct, RowSegments::FewestStaged);
        if (g.xpieces > 25) throw std::invalid_argument("conv_wgrad_rect: image segment too large for this variant");
        const int ct = g.mtiles * g.ntiles * g.tgroups;
        // as many workgroups as fit at once: LDS ring per CU, <= 3 of 7-9 waves; >= 4 segments per split
        const int occ = std::max(1, std::min(3, 160 * 1024 / (pl.stages * g.stage)));
        split_k(pl, g.nseg, std::max(1, (256 * occ + ct / 2) / ct), 4);
        g.splits = pl.splits, g.kps = pl.kps;
        pl.ws_floats = pl.splits > 1 ? static_cast<int64_t>(pl.splits) * s.Cout * g.taps * s.Cin : 0;
        return pl;
    }
    if (variant == kWgradRows) {
        if (s.stride != 1 || !conv_wgrad_rows_rect_supported(s)) throw std::invalid_argument(no_rows);
        WgradPlan pl = plan_of(WgradFamily::Rect, variant);
        RRGeo &g = pl.rect = rows_rect_geo(s, pl.ct, RowSegments::PixelRow);
        const int ct = g.mtiles * g.ntiles * g.tgroups;
        // ~2 workgroups of 7-9 waves per CU, >= 4 segments per split
        split_k(pl, g.nseg, std::max(1, (512 + ct / 2) / ct), 4);
        g.splits = pl.splits, g.kps = pl.kps;
        pl.ws_floats = pl.splits > 1 ? static_cast<int64_t>(pl.splits) * g.tiles * 4096 : 0;
        return pl;
    }
    // any other code: the tap-tiled kernel on the tile the channel counts pick
    WgradPlan pl = plan_of(WgradFamily::Rect, rect_tile(s));
    WGeo &g = pl.tiled = tiled_geo(s, pl);
    const int ksteps = static_cast<int>((s.P() + kBK - 1) / kBK);
    const int nw = pl.wm * pl.wn;
    const int target = 256 * (nw >= 4 ? 1 : 2) * (g.taps > 1 ? 2 : 1);
    split_k(pl, ksteps, (target + g.tiles / 2) / g.tiles, 4);
    g.splits = pl.splits, g.kps = pl.kps;
    pl.ws_floats = pl.splits > 1 ? static_cast<int64_t>(pl.splits) * g.tiles * pl.bm() * pl.bn() : 0;
    return pl;
}

}  // namespace

const char *wgrad_kernel_name(WgradKernel k) {
    switch (k) {
    case WgradKernel::Tiled: return "Tiled";
    case WgradKernel::Rows3x3: return "Rows3x3";
    case WgradKernel::RowsRect: return "RowsRect";
    default: return "RowsRing";
    }
}

const char *wgrad_route_name(WgradRoute r) {
    return r == WgradRoute::Library ? "library" : r == WgradRoute::Square ? "square" : "rect";
}

bool conv_wgrad_supported(int Cin, int Cout, int ks, int stride) {
    return (ks == 1 || ks == 3) && (stride == 1 || stride == 2) && Cin % 64 == 0 && Cout % 64 == 0 && Cin >= 64 &&
           Cout >= 64;
}

bool conv_wgrad_rect_supported(int Cin, int Cout, int kh, int kw, int stride) {
    return Cin % 8 == 0 && Cout % 8 == 0 && Cin >= 16 && Cout >= 16 && (stride == 1 || stride == 2) && kh >= 1 &&
           kw >= 1 && kh * kw <= 49;
}

bool conv_wgrad_rows_rect_supported(const WgradShape &s) {
    if ((s.stride != 1 && s.stride != 2) || s.taps() < 2 || !conv_wgrad_rect_supported(s.Cin, s.Cout, s.kh, s.kw, s.stride))
        return false;
    if (s.H + 2 * s.ph - s.kh < 0 || s.W + 2 * s.pw - s.kw < 0) return false;
    if (s.stride == 1) return rows_rect_geo(s, 64, RowSegments::PixelRow).xpieces <= 25;
    // stride 2: the ring variants only (64-channel tiles bound the staged image)
    return rows_rect_geo(s, 64, RowSegments::FewestStaged).xpieces <= 25;
}

// From the Inception-v3 sweep (profiles/r5_inception_wgrad.md): 32-channel tiles when both channel
// counts fit one; the 64-tile kernel on pixel-row segments when both are multiples of 64; otherwise
// 64-channel tiles on the fewest-rows segments with a 4-stage ring on the small maps (<= 32 x 32: few
// segments per workgroup, the ring's depth pays) when it fits in 96 KB, else a 3-stage ring (two
// workgroups per CU on the 54 x 54 / 109 x 109 maps)
int conv_wgrad_rows_rect_auto(const WgradShape &s) {
    if (s.Cin <= 32 && s.Cout <= 32) return kWgradRing32x2;
    const bool both64 = s.Cin % 64 == 0 && s.Cout % 64 == 0;
    if (s.stride == 2) {
        // stride-2 sweep: 25x25 96->96 34 us on 32x4 (MIOpen 50), 288->384 241 on 32x2 (tap-tiled 266,
        // MIOpen 324), 12x12 192->192 / 192->320 33 / 41 on 64x4 (MIOpen 29 / 41)
        if (!both64) return (s.H * s.W <= 1024 && s.Cout <= 128) ? kWgradRing32x4 : kWgradRing32x2;
        return kWgradRing64x4;
    }
    if (s.stride == 1 && both64) return kWgradRows;
    const RRGeo g = rows_rect_geo(s, 64, RowSegments::FewestStaged);
    return (s.H * s.W <= 1024 && 4 * g.stage <= 96 * 1024) ? kWgradRing64x4 : kWgradRing64x3;
}

WgradPlan conv_wgrad_plan(const WgradShape &s, WgradFamily family, int variant, int splits) {
    WgradPlan pl = family == WgradFamily::Square ? plan_square(s, variant, splits) : plan_rect(s, variant);
    pl.shape = s;
    return pl;
}

// Measured per shape against MIOpen (tools/bench_wgrad.py, tools/bench_inception_wgrad.py,
// profiles/r3q_inception_wgrad.txt, profiles/r5_inception_wgrad.md).
WgradRouting conv_wgrad_route(const WgradShape &s) {
    const WgradRouting library{WgradRoute::Library, kWgradAuto, 0};
    const int cin = s.Cin, cout = s.Cout;
    // square windows with their "same" padding and channel counts % 64: the square family's planner
    // (ResNet-tuned: the 3x3 row-image kernel etc.), or the library where it has no kernel
    if (s.kh == s.kw && s.ph == s.pw && s.ph == (s.kh - 1) / 2 && cin % 64 == 0 && cout % 64 == 0) {
        if (!conv_wgrad_supported(cin, cout, s.kh, s.stride)) return library;
        const WgradPlan pl = plan_square(s, kWgradAuto, -1);
        return {WgradRoute::Square, pl.variant, pl.kernel == WgradKernel::Rows3x3 ? kRowsMaxPixels : kTiledMaxPixels};
    }
    // the narrow stride-1 multi-tap windows (<= 192 inputs) and every stride-2 multi-tap window the
    // row-image kernels cover: all taps of a workgroup share one staged input image (54x54 80->192 3x3
    // 992 -> 405 us, 111x111 32->32 3x3 438 -> 167 us, 12x12 160->160 1x7 79 -> 55 us vs MIOpen; stride 2
    // 25x25 96->96 34 vs MIOpen 50 us, 288->384 241 vs 266 tap-tiled)
    if (s.taps() > 1 && (s.stride == 2 || (s.stride == 1 && cin <= 192)) && conv_wgrad_rows_rect_supported(s))
        return {WgradRoute::Rect, conv_wgrad_rows_rect_auto(s), kRowsMaxPixels};
    // the tap-tiled split-K kernel wins every 1x1 (2-3x) and the multi-tap windows over >= 256 input
    // channels; no batch chunking on this family: past the kernel's pixel cap the library takes it
    const bool wide = s.taps() == 1 || cin % 128 == 0 || cin >= 256;
    if (wide && std::min(cin, cout) >= 32 && conv_wgrad_rect_supported(cin, cout, s.kh, s.kw, s.stride) &&
        s.P() < kTiledMaxPixels)
        return {WgradRoute::Rect, rect_tile(s), kTiledMaxPixels};
    return library;
}

WgradReduceLaunch wgrad_reduce_launch(int64_t total4, int splits) {
    int sgl = 0;
    while (sgl < 6 && (2 << sgl) <= splits && (total4 << (sgl + 1)) <= int64_t(256) * 2048) ++sgl;
    const int64_t outs = 256 >> sgl;
    return {sgl, static_cast<int>((total4 + outs - 1) / outs)};
}

}  // namespace kfk
