// rt_denoise_plan.hpp -- how one feature-guided a-trous denoise (rtEnqueueDenoise) is launched, as a
// pure function of plain values (rt_denoise_plan.cpp): no HIP, no allocation, no globals.  The C ABI
// fills a DenoiseIn, calls denoise_plan, grows the kernel's scratch to scratch_pixels and launches
// one kernel per DenoiseStep (rt_denoise.hip).
//
// The tile of a step-s iteration: kDenoiseTileW contiguous columns of `rows` image rows taken at
// stride s, all of one residue class y mod s.  A tap of pixel (x, y) is (x + s dx, y + s dy), so the
// tile's taps lie in the same class: the staged block is (kDenoiseTileW + 4 s) columns of rows + 4
// class rows, every row x-contiguous in memory.  Workgroup b of the 1-D grid is tile
// (b % tiles_x, (b / tiles_x) % tiles_per_class) of class b / (tiles_x * tiles_per_class); class c
// holds rows c, c + s, ... and its tile t rows c + (t rows + j) s, j < rows.  Classes with fewer rows
// than class 0 leave their last tile empty.
#pragma once

#include <stddef.h>
#include <stdint.h>

// A/B switches (scripts/build_variant.sh): rows of a tile at steps 1 .. 8 and at step 16, and the
// workgroup size (a multiple of 64).  The defaults are the measured choice.
#ifndef RT_DENOISE_ROWS
#define RT_DENOISE_ROWS 8
#endif
#ifndef RT_DENOISE_ROWS_FAR
#define RT_DENOISE_ROWS_FAR 4
#endif
#ifndef RT_DENOISE_THREADS
#define RT_DENOISE_THREADS 512
#endif

namespace rtp {

constexpr unsigned kDenoiseMaxIterations = 5;
constexpr uint64_t kDenoiseMaxPixels = 1ull << 31;    // pixel indices are 32-bit
constexpr uint32_t kDenoiseTileW = 64;                // columns of a tile: one wave's lanes
constexpr uint32_t kDenoiseThreads = RT_DENOISE_THREADS;  // 64 columns x 8 rows per pass
constexpr uint32_t kDenoiseCellBytes = 48;            // staged per cell: colour, {albedo, depth}, {normal, coverage}
constexpr uint32_t kDenoisePadBytes = 64;             // between the two feature planes (bank offset of the staging stores)
constexpr uint32_t kDenoisePixelBytes = 16, kDenoiseFeatureBytes = 32;
constexpr size_t kDenoiseLdsBudget = 64 * 1024;       // static LDS of one workgroup
// [2^-20, 2^20]: every 1 / sigma^2 is finite, the halved colour tolerances of 5 iterations included
constexpr float kDenoiseSigmaMin = 0x1p-20f, kDenoiseSigmaMax = 0x1p20f;

enum DenoiseBuf { kDenoiseImage = 0, kDenoiseOut = 1, kDenoiseScratch = 2 };
enum DenoiseTerm { kDenoiseColor = 1, kDenoiseNormal = 2, kDenoiseDepth = 4, kDenoiseAlbedo = 8 };

// rows of a tile at step s: 8 where the staged block fits the budget, else 4 (step 16)
constexpr uint32_t denoise_rows(uint32_t step) { return step >= 16 ? RT_DENOISE_ROWS_FAR : RT_DENOISE_ROWS; }

struct DenoiseIn {
    bool params_ok;                      // params != NULL
    unsigned iterations;
    float sigma_color, sigma_normal, sigma_depth, sigma_albedo;
    uint64_t width, height;
    bool image_ok, features_ok, out_ok;  // each a buffer of this context
    bool out_is_input;                   // `out` is `image` or `features`
    uint64_t image_bytes, features_bytes, out_bytes;
};

struct DenoiseStep {
    uint32_t step;                       // 2^i
    int src, dst;                        // DenoiseBuf
    float inv_c;                         // 1 / ldexpf(sigma_color, -i)^2 (0 when the term is off)
    uint32_t rows;                       // image rows of a tile
    uint32_t stage_w, stage_h;           // staged cells: kDenoiseTileW + 4 step columns, rows + 4 class rows
    uint32_t lds_bytes;
    uint32_t tiles_x, classes, tiles_per_class;
    uint32_t grid;                       // workgroups of kDenoiseThreads
};

struct DenoisePlan {
    unsigned iterations;
    uint32_t width, height;
    uint64_t scratch_pixels;             // the ping-pong image (0: not needed)
    uint32_t terms;                      // DenoiseTerm bits of the enabled edge-stopping terms
    float inv_n, inv_z, inv_a;           // 1 / sigma^2 (0 when the term is off)
    DenoiseStep it[kDenoiseMaxIterations];
};

// RT_SUCCESS, or, in this order: RT_INVALID_VALUE (no params; iterations outside 1..5; a sigma that is
// negative, not finite, in (0, 2^-20) or above 2^20; width or height zero; width * height > 2^31),
// RT_INVALID_MEM_OBJECT (a buffer that is NULL or another context's; `out` one of the inputs),
// RT_INVALID_BUFFER_SIZE (image or out below 16 B per pixel, features below 32 B).
int denoise_plan(const DenoiseIn& in, DenoisePlan* out);

// ---- rtEnqueueDenoiseSamples: the variance-guided filter over the adaptive sample statistics ------
// The tiles, the rows per step and the alternation of the buffers are denoise_plan's: the staged cell is
// the same 48 B (the colour plane's w slot carries the variance), so the LDS of a step is too.  The
// first iteration stages from the statistics (kDenoiseImage stands for them), the last one encodes,
// reads the sample counts and writes the variance plane.
constexpr uint32_t kDenoiseStatsBytes = 32, kDenoiseVarianceBytes = 4;
constexpr float kDenoiseEpsilonMin = 0x1p-40f, kDenoiseEpsilonMax = 0x1p20f;
constexpr int kDenoiseLinear = 0, kDenoiseGamma = 1;  // RT_DENOISE_LINEAR, RT_DENOISE_GAMMA
constexpr uint32_t kDenoiseLuminance = kDenoiseColor;  // the luminance term takes the colour term's bit

struct DenoiseSamplesIn {
    bool params_ok;                      // params != NULL
    unsigned iterations;
    float sigma_luminance, sigma_normal, sigma_depth, sigma_albedo, epsilon;
    int encoding;
    uint64_t width, height;
    bool stats_ok, features_ok, out_ok;  // each a buffer of this context
    bool variance_given, variance_ok;    // `variance` is not NULL; ... and a buffer of this context
    bool aliased;                        // `out` or `variance` is an input, or they are each other
    uint64_t stats_bytes, features_bytes, out_bytes, variance_bytes;
};

struct DenoiseSamplesPlan {
    unsigned iterations;
    uint32_t width, height;
    uint64_t scratch_pixels;             // the ping-pong image (0: not needed)
    uint32_t terms;                      // DenoiseTerm bits of the enabled terms (kDenoiseLuminance for the first)
    float sigma_luminance, epsilon;
    float inv_n, inv_z, inv_a;           // 1 / sigma^2 (0 when the term is off)
    int encoding;
    bool write_variance;
    DenoiseStep it[kDenoiseMaxIterations];  // (inv_c is not used: 0)
    bool first[kDenoiseMaxIterations];   // stages from the statistics: iteration 0 alone
    bool last[kDenoiseMaxIterations];    // writes the encoded image, the counts and the variance: the last alone
};

// RT_SUCCESS, or, in this order: RT_INVALID_VALUE (no params; iterations outside 1..5; a sigma that is
// negative, not finite, in (0, 2^-20) or above 2^20; epsilon not finite or outside [2^-40, 2^20]; an
// encoding other than the two; width or height zero; width * height > 2^31), RT_INVALID_MEM_OBJECT (a
// required buffer that is NULL or another context's; a `variance` of another context; `out` or
// `variance` an input or each other), RT_INVALID_BUFFER_SIZE (stats or features below 32 B per pixel,
// out below 16 B, variance below 4 B).
int denoise_samples_plan(const DenoiseSamplesIn& in, DenoiseSamplesPlan* out);

}  // namespace rtp
