// lde_plan.h -- which kernel runs each of the three passes of lde_table (ntt.hip), with its launch shape: a pure function of the
// table's shape.  Plain C++17 (no HIP, no context): ntt.hip launches from it, tests/lde_plan_dump.cpp prints it.  DESIGN.md 4.1 has
// the resulting table of kernels per trace height; this file is the authority.
#pragma once
#include <cstddef>
#include <cstdint>

// ---- LDS layouts shared by the kernels (ntt.hip) and the plan ----------------------------------------------------------------
#define TVM_ROW_PAD 1   // the tile kernels: element (a, b) of 2^b transforms side by side at s[a + b * (n + TVM_ROW_PAD)]
#define TVM_ROW_WORDS(n) ((n) + ((n) >> 4) + 1)   // odd pitch: position p of the 16 rows of a tile falls into 16 different banks
// k_lde_pass2_fused:
#define TVM_P2F_ROWW(logn) ((logn) == 8 ? 296 : (logn) == 9 ? 552 : (logn) == 10 ? 1096 : 2184)   // >= TVM_ROW_WORDS, = 8 (mod 32)
#define TVM_P2F_TW2_WORDS 272   // 16 x 17: the middle group's twiddles
#define TVM_P2F_LDS_WORDS(logn) (8 * TVM_P2F_ROWW(logn) + TVM_P2F_TW2_WORDS + TVM_ROW_WORDS(1 << (logn)) + 8)
#define TVM_P2F_FLAG_WORDS 512   // u64 words in front of the tile at 2048 points: sixteen blocks of 64 pair flags (tvm_pair_sync)
#define TVM_P2F_LDS_BYTES(logn) ((size_t)(TVM_P2F_LDS_WORDS(logn) + ((logn) == 11 ? TVM_P2F_FLAG_WORDS : 0)) * sizeof(std::uint64_t))   // tile + twiddles + one coset's factors + a randomizer word per row: 79.2 / 159.4 KB
// the pass split at the coefficients (LdePass2Args::mode)
#define TVM_LDE_INVERSE_ONLY 1
#define TVM_LDE_FORWARD_ONLY 2

namespace tvm {

// One enumerator per kernel instantiation that ntt.hip launches, in the order of its table of variants (g_variants).
enum class LdeKernel : int {
    none = -1,   // the pass is not run (a split mode skips it)
    ntt2_pass1, ntt2_pass2,   // the generic column / row step (k_ntt2_pass2: ntt_columns only, never part of a plan)
    lde_pass2, lde_pass3,     // the generic middle / last pass
    pass1_rows_8_16, pass1_rows_9_16, pass1_rows_10_16, pass1_rows_11_8,
    pass2_fused_8, pass2_fused_9, pass2_fused_10, pass2_fused_11,
    pass2_v3_7_6, pass2_v3_8_6, pass2_v3_11_10, pass2_v3_12_10,
    pass3_rows_8_8, pass3_rows_9_8, pass3_rows_10_8, pass3_rows_11_8, pass3_halves_8,
    pass3_v3_7_6, pass3_v3_8_6, pass3_v3_12_10,
    count
};

inline bool is_pass2_fused(LdeKernel k) { return k >= LdeKernel::pass2_fused_8 && k <= LdeKernel::pass2_fused_11; }

struct LdePlanInput {
    int log_n;            // the trace has 2^log_n rows, split n1 x n2 with log_n1 = log_n / 2 (rounded down)
    std::uint64_t X;      // cosets (expansion factor)
    std::uint64_t h;      // trace randomizers per column
    bool std_roots;       // the trace generator is the domains' own root of unity (classify_root)
    int tiles_option;     // TVM_OPTION_LDE_PASS2_TILES
    int mode;             // 0, TVM_LDE_INVERSE_ONLY (no pass 3) or TVM_LDE_FORWARD_ONLY (no pass 1)
};

struct LdePass {
    LdeKernel kernel = LdeKernel::none;
    int block = 0;               // work-items per workgroup
    std::size_t lds_bytes = 0;   // dynamic LDS
    int rows = 0;                // rows per tile: the grid is ceil(rows of the pass / rows) x columns ...
    int tiles = 0;               // ... except pass 3's row and tile kernels: `tiles` consecutive tiles per workgroup,
    std::uint64_t grid_y = 0;    //     grid = columns x grid_y (to be checked against the 65535 of a grid's second dimension)
};
struct LdePlan {
    LdePass pass1, pass2, pass3;
};

// ---- pass 1's row kernels of 16-row tiles (k_lde_pass1_rows<8 | 9 | 10, 16>): persistent workgroups --------------------------------
// A launch has `columns` x 2^log_tiles work items (column, tile), numbered tile-fastest inside a column; workgroup g of G walks the
// items g, g + G, g + 2 G, ... -- the workgroups that run together read neighbouring 128-byte runs of one column -- and has the
// input of its next item, if it has one, in flight while it transforms the current one.  These functions are the numbering: the kernel and the
// host launch from them, tests/lde_pass1_grid_dump.cpp walks them.
#if defined(__HIPCC__)
#define TVM_PLAN_FN __host__ __device__ inline
#else
#define TVM_PLAN_FN inline
#endif
struct LdePass1Item {
    std::uint64_t column, tile;
};
TVM_PLAN_FN std::uint64_t lde_pass1_items(std::uint64_t columns, int log_tiles) { return columns << log_tiles; }
TVM_PLAN_FN LdePass1Item lde_pass1_item(std::uint64_t index, int log_tiles) {
    return {index >> log_tiles, index & (((std::uint64_t)1 << log_tiles) - 1)};
}

inline int threads_for_tile(int tile) {
    int t = tile / 16;
    t = (t + 63) / 64 * 64;
    if (t < 64) t = 64;
    if (t > 1024) t = 1024;
    return t;
}
// Tile = 2^log_axis points x 2^batch transforms, at most 2^14 words = 128 KiB of LDS (one 1024-thread workgroup per
// CU).  Measured alternative: 64 KiB tiles with two 512-thread workgroups per CU, so that one workgroup's global
// traffic overlaps the other's butterflies -- no gain for the generic passes in round 1 (24.9 vs 25.5 ms for 128
// columns), but worth 4 % for the LDE's pass 3 once its arithmetic had been trimmed (lde_table: k_lde_pass3_v3<10, 9>).
inline int tile_words_log() { return 14; }
inline int batch_log_for(int log_axis) {
    int b = tile_words_log() - log_axis;
    if (b < 0) b = 0;
    return b > 4 ? 4 : b;
}
// the generic kernels: 2^batch_log transforms of 2^log_axis points per workgroup, `pad` words between two of them
inline LdePass lde_generic_pass(LdeKernel kernel, int log_axis, int batch_log, int pad) {
    LdePass p;
    p.kernel = kernel;
    p.block = threads_for_tile((1 << log_axis) << batch_log);
    p.lds_bytes = ((std::size_t)((1 << log_axis) + pad) << batch_log) * sizeof(std::uint64_t);
    p.rows = 1 << batch_log;
    return p;
}

// Workgroups of a launch of pass 1's persistent row kernels over `items` work items: option (TVM_OPTION_LDE_PASS1_WORKGROUPS) of them,
// never more than there are items.  0 and any count at or above the items: ONE tile per workgroup, no second trip through the loop.
// (Measured at 2^20 rows with a workgroup per compute unit, 256 for 6144 items: the kernel -13 %.  A context starts with its device's
// compute-unit count -- context.hip, the one unit that asks the device; this header only does the arithmetic: DESIGN.md 9.)
inline std::uint64_t lde_pass1_workgroups(std::uint64_t items, std::uint64_t option) {
    const std::uint64_t g = option ? option : items;
    return g < items ? g : (items ? items : 1);
}
inline bool is_pass1_persistent(LdeKernel k) { return k >= LdeKernel::pass1_rows_8_16 && k <= LdeKernel::pass1_rows_10_16; }

inline LdePlan lde_plan(const LdePlanInput& in) {
    const int log_n1 = in.log_n / 2, log_n2 = in.log_n - log_n1;   // (so n2 >= n1: an axis long enough for a row or tile kernel
    const std::size_t n1 = (std::size_t)1 << log_n1, n2 = (std::size_t)1 << log_n2;   // always has whole tiles on the other axis)
    const std::uint64_t rows3_total = in.X * n2;   // pass 3 transforms a row per coset and j1
    // TVM_OPTION_LDE_PASS2_TILES = 1 takes away: k_lde_pass2_fused on every axis, the row kernels of passes 1 and 3 on 256-, 512-
    // and 2048-point axes, k_lde_pass3_halves.  The row kernels of passes 1 and 3 on 1024-point axes run with either value.
    const bool row_kernels_allowed = in.tiles_option == 0;
    const auto pass = [](LdeKernel kernel, int block, std::size_t lds_words, int rows) {
        LdePass p;
        p.kernel = kernel;
        p.block = block;
        p.lds_bytes = lds_words * sizeof(std::uint64_t);
        p.rows = rows;
        return p;
    };
    const auto tile_pass = [&](LdeKernel kernel, int block, std::size_t axis, bool pass2) {   // k_lde_pass{2,3}_v3
        const int rows = 16 * block / (int)axis;
        return pass(kernel, block, rows * (axis + TVM_ROW_PAD) + (axis < 4096 ? axis : 0) + (pass2 ? 32 : 0), rows);
    };
    LdePlan plan;

    // pass 1: a row per 16 / 32 / 64 lanes (256 / 512 / 1024 points), 16 rows and a row of twiddles; 2048 points: two wavefronts per
    // row, 8 rows, sixteen blocks of 64 pair flags in front.
    // (1024 points, 16-row tiles: 128-byte runs of the input.  8-row tiles -- two workgroups per CU, one's loads under the other's
    // butterflies -- measured the same time and fetch every input line twice: 16 instead of 8 B per cell, profiles/r03_q_pmc_lde.txt.
    // The 16-row kernels can overlap within ONE workgroup instead -- fewer workgroups than tiles, the next tile in registers:
    // lde_pass1_workgroups.)
    if (in.mode != TVM_LDE_FORWARD_ONLY) {
        const std::size_t words16 = 16 * TVM_ROW_WORDS(n1) + n1;
        if (in.std_roots && log_n1 == 8 && row_kernels_allowed) plan.pass1 = pass(LdeKernel::pass1_rows_8_16, 256, words16, 16);
        else if (in.std_roots && log_n1 == 9 && row_kernels_allowed) plan.pass1 = pass(LdeKernel::pass1_rows_9_16, 512, words16, 16);
        else if (in.std_roots && log_n1 == 10) plan.pass1 = pass(LdeKernel::pass1_rows_10_16, 1024, words16, 16);
        else if (in.std_roots && log_n1 == 11 && row_kernels_allowed)
            plan.pass1 = pass(LdeKernel::pass1_rows_11_8, 1024, 8 * TVM_ROW_WORDS(n1) + n1 + 512, 8);
        else plan.pass1 = lde_generic_pass(LdeKernel::ntt2_pass1, log_n1, batch_log_for(log_n1), 0);
    }

    // pass 2.  256 .. 2048-point axes: every wavefront (pair of wavefronts) keeps its rows across the coset loop (k_lde_pass2_fused,
    // 8 rows per tile); more trace randomizers than n1 (never the case for a STARK's parameters) take the kernels below.
    // Axes longer than a workgroup: 2048 / 4096 points on 1024 work-items (k_lde_pass2_v3; 2^21 .. 2^24 rows), and the same shapes at
    // a size the CPU suite can run (128 / 256 points on 64 work-items); rows per tile = 16 / positions per work-item.
    // Anything else: the generic kernel, whose tile height lde_table narrows for short traces (it needs the column count).
    {
        const std::size_t fused_words = TVM_P2F_LDS_BYTES(log_n2) / sizeof(std::uint64_t);
        const bool fused = in.std_roots && row_kernels_allowed && in.h <= n1;
        if (fused && log_n2 == 8) plan.pass2 = pass(LdeKernel::pass2_fused_8, 128, fused_words, 8);
        else if (fused && log_n2 == 9) plan.pass2 = pass(LdeKernel::pass2_fused_9, 256, fused_words, 8);
        else if (fused && log_n2 == 10) plan.pass2 = pass(LdeKernel::pass2_fused_10, 512, fused_words, 8);
        else if (fused && log_n2 == 11) plan.pass2 = pass(LdeKernel::pass2_fused_11, 1024, fused_words, 8);
        else if (in.std_roots && log_n2 == 7) plan.pass2 = tile_pass(LdeKernel::pass2_v3_7_6, 64, n2, true);
        else if (in.std_roots && log_n2 == 8) plan.pass2 = tile_pass(LdeKernel::pass2_v3_8_6, 64, n2, true);
        else if (in.std_roots && log_n2 == 11) plan.pass2 = tile_pass(LdeKernel::pass2_v3_11_10, 1024, n2, true);
        else if (in.std_roots && log_n2 == 12) plan.pass2 = tile_pass(LdeKernel::pass2_v3_12_10, 1024, n2, true);
        else plan.pass2 = lde_generic_pass(LdeKernel::lde_pass2, log_n2, batch_log_for(log_n2), TVM_ROW_PAD);
    }

    // pass 3.  256 .. 2048-point axes: one (k, j1) row per wavefront, no workgroup barrier (k_lde_pass3_rows): 8 wavefronts per
    // workgroup -- 78 KB of LDS, two workgroups per CU at 1024 points (4 wavefronts per workgroup: +2 %, 16: +3 %,
    // profiles/r03_g_lde_ab.txt); one workgroup per CU at 2048, where the default is the row as two 1024-point halves through one
    // LDS region per wavefront (k_lde_pass3_halves).
    // (pass 3 has no coset loop and no workgroup barrier: here the 2048-point row form is 8 % faster than k_lde_pass3_v3<11, 10>,
    // 15.5 against 16.8 ms per 96 columns at 2^22 rows, even at two wavefronts per SIMD -- that instantiation is launched nowhere)
    // 128 / 256 / 4096 points: the tile kernels, as in pass 2.  Anything else, an axis nobody foresaw included: the generic kernel.
    if (in.mode != TVM_LDE_INVERSE_ONLY) {
        const std::size_t words8 = 8 * TVM_ROW_WORDS(n1) + n1;
        LdePass& p = plan.pass3;
        if (in.std_roots && log_n1 == 8 && row_kernels_allowed) p = pass(LdeKernel::pass3_rows_8_8, 512, words8, 8);
        else if (in.std_roots && log_n1 == 9 && row_kernels_allowed) p = pass(LdeKernel::pass3_rows_9_8, 512, words8, 8);
        else if (in.std_roots && log_n1 == 10) p = pass(LdeKernel::pass3_rows_10_8, 512, words8, 8);
        else if (in.std_roots && log_n1 == 11 && row_kernels_allowed) p = pass(LdeKernel::pass3_halves_8, 512, 8 * TVM_ROW_WORDS(1024) + 1024, 8);
        else if (in.std_roots && log_n1 == 11) p = pass(LdeKernel::pass3_rows_11_8, 512, words8, 8);
        else if (in.std_roots && log_n1 == 7) p = tile_pass(LdeKernel::pass3_v3_7_6, 64, n1, false);
        else if (in.std_roots && log_n1 == 8) p = tile_pass(LdeKernel::pass3_v3_8_6, 64, n1, false);
        else if (in.std_roots && log_n1 == 12) p = tile_pass(LdeKernel::pass3_v3_12_10, 1024, n1, false);
        else p = lde_generic_pass(LdeKernel::lde_pass3, log_n1, batch_log_for(log_n1), TVM_ROW_PAD);
        if (p.kernel != LdeKernel::lde_pass3) {   // consecutive tiles per workgroup: up to 16 of the row kernels', 8 of the tile kernels'
            const std::uint64_t tiles_total = rows3_total / p.rows;
            p.tiles = 1;
            for (int t = p.block == 512 ? 16 : 8; t >= 4; t /= 2)
                if (tiles_total % t == 0) { p.tiles = t; break; }
            p.grid_y = tiles_total / p.tiles;
        }
    }
    return plan;
}

}  // namespace tvm
