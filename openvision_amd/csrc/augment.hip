// augment.hip — the training image transform on the device, one call per batch of variable-sized images, gfx950.
//
// Replaces the training branch of open_clip.transform.image_transform (src/convert_upload/open_clip/transform.py:307-358):
//     RandomResizedCrop(size, scale, BICUBIC) -> _convert_to_rgb -> [color_jitter] -> [gray_scale] -> ToTensor -> Normalize
// on PIL images, i.e. Pillow's img.crop(box).resize(...) (src/libImaging/Resample.c), ImageEnhance.Brightness / Contrast / Color
// (Image.blend against a degenerate image, src/libImaging/Blend.c) and convert("L") (src/libImaging/Convert.c).  The random numbers
// (the crop boxes, the order and factors of the colour operations) are drawn on the host (openvision_amd/augment.py); everything
// after them is computed here in Pillow's own arithmetic, so the uint8 image equals Pillow's bit for bit.
//
// A fixed number of launches whatever the batch size, nothing synchronises with the host:
//   tt_plan        Resample.c precompute_coeffs + normalize_coeffs_8bpc in fp64, per image and axis, for crop extent -> output size
//   tt_resample_h  horizontal pass over every image's crop rows (grid z = image, y = crop row; rows past an image's crop exit)
//   tt_resample_v  vertical pass, writes the resized uint8 [B, out_h, out_w, 3]
//   tt_luma_sum    only when an image has a contrast operation: exact integer sum of L after the operations that precede it
//   tt_finish      the colour operations in order, x / 255, (x - mean) / std, CHW fp32 or bf16
// The resample arithmetic is that of preprocess.hip (int32 accumulation from 1 << 21, >> 22, clip, uint8 between the passes).
//
// Pillow's results depend on every product and sum being rounded on its own (the planner's doubles, the blend's floats), so
// floating-point contraction is off for this whole file.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;      // Resample.c

// ---- the workspace, stated once ------------------------------------------------------------------------------------------------
struct TtLayout {
    size_t sums, bounds_x, taps_x, bounds_y, taps_y, htmp, resized, total;
};
TtLayout tt_layout(int B, int out_h, int out_w, int max_rows, int max_taps_x, int max_taps_y) {
    TtLayout l;
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t o = at;
        at += (bytes + 15) & ~(size_t)15;
        return o;
    };
    l.sums = take((size_t)B * 4 * sizeof(unsigned long long));            // sum of L per image and operation slot
    l.bounds_x = take((size_t)B * out_w * 2 * sizeof(int));
    l.taps_x = take((size_t)B * out_w * max_taps_x * sizeof(int));
    l.bounds_y = take((size_t)B * out_h * 2 * sizeof(int));
    l.taps_y = take((size_t)B * out_h * max_taps_y * sizeof(int));
    l.htmp = take((size_t)B * max_rows * out_w * 3);                      // horizontal intermediate, uint8
    l.resized = take((size_t)B * out_h * out_w * 3);                      // resized crop, uint8
    l.total = at;
    return l;
}

// ---- planner -------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
__host__ __device__ __forceinline__ double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// one output position of one axis: bounds[0..1] = (first source index, tap count), taps[0..max_taps) zero padded
// (host-callable as well: tools/plan_host_check.py holds the arithmetic against preprocess.resize_plan on the CPU)
template <bool CUBIC>
__host__ __device__ void plan_row(int in_size, int out_size, int xx, int max_taps, int* __restrict__ bounds, int* __restrict__ taps) {
    int xmin = 0, xmax = 0;
    double center = 0.0, ss = 1.0, ww = 0.0;
    if (in_size > 0) {
        const double scale = (double)in_size / (double)out_size;
        const double filterscale = scale >= 1.0 ? scale : 1.0;
        const double support = (CUBIC ? 2.0 : 1.0) * filterscale;
        ss = 1.0 / filterscale;
        center = 0.0 + (xx + 0.5) * scale;
        xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        if (xmax > max_taps) xmax = max_taps;       // never with the caller's max_taps >= this extent's ksize; keeps the row in bounds
        if (xmax < 0) xmax = 0;
        for (int x = 0; x < xmax; ++x) {
            const double arg = (x + xmin - center + 0.5) * ss;
            ww += CUBIC ? bicubic_filter(arg) : bilinear_filter(arg);
        }
    }
    for (int x = 0; x < max_taps; ++x) {
        int k = 0;
        if (x < xmax) {
            const double arg = (x + xmin - center + 0.5) * ss;
            double v = CUBIC ? bicubic_filter(arg) : bilinear_filter(arg);
            if (ww != 0.0) v = v / ww;
            k = v < 0 ? (int)(-0.5 + v * (double)(1 << PRECISION_BITS)) : (int)(0.5 + v * (double)(1 << PRECISION_BITS));
        }
        taps[x] = k;
    }
    bounds[0] = xmin;
    bounds[1] = xmax;
}

template <bool CUBIC>
__global__ __launch_bounds__(256) void tt_plan(const int* __restrict__ boxes, int B, int out_h, int out_w, int max_taps_x,
                                               int max_taps_y, int* __restrict__ bounds_x, int* __restrict__ taps_x,
                                               int* __restrict__ bounds_y, int* __restrict__ taps_y,
                                               unsigned long long* __restrict__ sums) {
    const int per = out_w + out_h;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * per) return;
    const int b = (int)(i / per), t = (int)(i % per);
    if (sums && t == 0)                           // the statistics launch adds into them later in the stream
        for (int j = 0; j < 4; ++j) sums[4 * b + j] = 0;
    if (t < out_w) {
        const int64_t r = (int64_t)b * out_w + t;
        plan_row<CUBIC>(boxes[4 * b + 3], out_w, t, max_taps_x, bounds_x + 2 * r, taps_x + r * max_taps_x);
    } else {
        const int64_t r = (int64_t)b * out_h + (t - out_w);
        plan_row<CUBIC>(boxes[4 * b + 2], out_h, t - out_w, max_taps_y, bounds_y + 2 * r, taps_y + r * max_taps_y);
    }
}

int launch_plan(const int* boxes, int B, int out_h, int out_w, int interpolation, int max_taps_x, int max_taps_y, int* bounds_x,
                int* taps_x, int* bounds_y, int* taps_y, unsigned long long* sums, hipStream_t st) {
    const int64_t threads = (int64_t)B * (out_w + out_h);
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (interpolation == OV_INTERP_BICUBIC)
        hipLaunchKernelGGL(tt_plan<true>, grid, dim3(256), 0, st, boxes, B, out_h, out_w, max_taps_x, max_taps_y, bounds_x, taps_x,
                           bounds_y, taps_y, sums);
    else
        hipLaunchKernelGGL(tt_plan<false>, grid, dim3(256), 0, st, boxes, B, out_h, out_w, max_taps_x, max_taps_y, bounds_x, taps_x,
                           bounds_y, taps_y, sums);
    OV_LAUNCH_CHECK();
    return OV_OK;
}

// ---- resample passes -----------------------------------------------------------------------------------------------------------
// An image's crop as the passes address it.  ok: the image lies inside the packed buffer, the box inside the image, and the crop's
// rows inside the horizontal intermediate.  The host checks all of it before the call; an image that fails here is never read and
// comes out as the normalised black image.
struct Crop {
    int64_t off;
    int W, top, left, h;
    bool ok;
};
__device__ __forceinline__ Crop load_crop(const int64_t* __restrict__ offsets, const int* __restrict__ shapes,
                                          const int* __restrict__ boxes, int64_t pixel_bytes, int max_rows, int b) {
    Crop c;
    const int H = shapes[2 * b];
    c.W = shapes[2 * b + 1];
    c.off = offsets[b];
    c.top = boxes[4 * b];
    c.left = boxes[4 * b + 1];
    c.h = boxes[4 * b + 2];
    const int w = boxes[4 * b + 3];
    c.ok = H > 0 && c.W > 0 && c.off >= 0 && c.top >= 0 && c.left >= 0 && c.h > 0 && w > 0 && c.h <= H - c.top && w <= c.W - c.left &&
           c.h <= max_rows && (int64_t)H * c.W * 3 <= pixel_bytes - c.off;
    return c;
}

__device__ __forceinline__ unsigned char clip8(int v) {
    v >>= PRECISION_BITS;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// htmp[b][y][xx][c] = clip8((1 << 21) + sum_x src[top + y][left + xmin + x][c] * k[xx][x]) for y in [0, h_b), xx in [0, out_w)
__global__ __launch_bounds__(256) void tt_resample_h(const unsigned char* __restrict__ pixels, int64_t pixel_bytes,
                                                     const int64_t* __restrict__ offsets, const int* __restrict__ shapes,
                                                     const int* __restrict__ boxes, const int* __restrict__ bounds,
                                                     const int* __restrict__ taps, int max_taps, unsigned char* __restrict__ htmp,
                                                     int max_rows, int out_w) {
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y, b = blockIdx.z;
    if (xx >= out_w) return;
    const Crop c = load_crop(offsets, shapes, boxes, pixel_bytes, max_rows, b);
    if (!c.ok || y >= c.h) return;
    const int64_t r = (int64_t)b * out_w + xx;
    const int xmin = bounds[2 * r], cnt = bounds[2 * r + 1];
    const int* k = taps + r * max_taps;
    const unsigned char* p = pixels + c.off + ((int64_t)(c.top + y) * c.W + c.left + xmin) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int x = 0; x < cnt; ++x) {
        const int w = k[x];
        s0 += (int)p[3 * x] * w;
        s1 += (int)p[3 * x + 1] * w;
        s2 += (int)p[3 * x + 2] * w;
    }
    unsigned char* o = htmp + (((int64_t)b * max_rows + y) * out_w + xx) * 3;
    o[0] = clip8(s0); o[1] = clip8(s1); o[2] = clip8(s2);
}

// resized[b][yo][xo][c] = clip8((1 << 21) + sum_y htmp[b][ymin + y][xo][c] * k[yo][y])
__global__ __launch_bounds__(256) void tt_resample_v(const unsigned char* __restrict__ htmp, int max_rows, int64_t pixel_bytes,
                                                     const int64_t* __restrict__ offsets, const int* __restrict__ shapes,
                                                     const int* __restrict__ boxes, const int* __restrict__ bounds,
                                                     const int* __restrict__ taps, int max_taps, unsigned char* __restrict__ resized,
                                                     int out_h, int out_w) {
    const int xo = blockIdx.x * blockDim.x + threadIdx.x;
    const int yo = blockIdx.y, b = blockIdx.z;
    if (xo >= out_w) return;
    unsigned char* o = resized + (((int64_t)b * out_h + yo) * out_w + xo) * 3;
    const Crop c = load_crop(offsets, shapes, boxes, pixel_bytes, max_rows, b);
    if (!c.ok) {
        o[0] = 0; o[1] = 0; o[2] = 0;
        return;
    }
    const int64_t r = (int64_t)b * out_h + yo;
    const int ymin = bounds[2 * r], cnt = bounds[2 * r + 1];          // ymin + cnt <= h_b <= max_rows (the planner clamps to the extent)
    const int* k = taps + r * max_taps;
    const unsigned char* p = htmp + (((int64_t)b * max_rows + ymin) * out_w + xo) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int y = 0; y < cnt; ++y) {
        const int w = k[y];
        const unsigned char* q = p + (int64_t)y * out_w * 3;
        s0 += (int)q[0] * w;
        s1 += (int)q[1] * w;
        s2 += (int)q[2] * w;
    }
    o[0] = clip8(s0); o[1] = clip8(s1); o[2] = clip8(s2);
}

// ---- colour stage --------------------------------------------------------------------------------------------------------------
// Convert.c rgb2l: L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16
__device__ __forceinline__ int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Blend.c ImagingBlend(degenerate, image, f) on one band: fp32, the product and the sum rounded separately; truncated for
// 0 <= f <= 1 (the result cannot leave [0, 255]), clipped and truncated otherwise
__device__ __forceinline__ int blend8(int d, int p, float f) {
    const float t = (float)d + f * (float)(p - d);
    if (f >= 0.0f && f <= 1.0f) return (int)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// an image's operations in application order, and for a contrast operation the sum of L it needs
struct ColorOps {
    int op[4];
    float f[4];
    unsigned long long sum[4];
};
__device__ __forceinline__ ColorOps load_ops(const int* __restrict__ ops, const float* __restrict__ factors,
                                             const unsigned long long* __restrict__ sums, int b) {
    ColorOps c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c.op[j] = ops[4 * b + j];
        c.f[j] = factors[4 * b + j];
        c.sum[j] = sums[4 * b + j];
    }
    return c;
}
// operations [0, upto) on one pixel; npix = out_h * out_w for ImageEnhance.Contrast's int(mean(L) + 0.5)
__device__ __forceinline__ void apply_ops(const ColorOps& c, int upto, double npix, int& r, int& g, int& b) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= upto) break;
        const float f = c.f[j];
        if (c.op[j] == OV_COLOR_BRIGHTNESS) {
            r = blend8(0, r, f); g = blend8(0, g, f); b = blend8(0, b, f);
        } else if (c.op[j] == OV_COLOR_CONTRAST) {
            const int m = (int)((double)c.sum[j] / npix + 0.5);
            r = blend8(m, r, f); g = blend8(m, g, f); b = blend8(m, b, f);
        } else if (c.op[j] == OV_COLOR_SATURATION) {
            const int l = luma(r, g, b);
            r = blend8(l, r, f); g = blend8(l, g, f); b = blend8(l, b, f);
        } else if (c.op[j] == OV_COLOR_GRAYSCALE) {
            r = g = b = luma(r, g, b);
        }
    }
}

// Pass `pass` serves each image's pass-th contrast operation (slot j): sums[b][j] = sum over the resized image of L after operations
// [0, j).  Integer, so the order of the adds does not matter: wave, then block, then one atomic add per block.
__global__ __launch_bounds__(256) void tt_luma_sum(const unsigned char* __restrict__ resized, const int* __restrict__ ops,
                                                   const float* __restrict__ factors, unsigned long long* __restrict__ sums,
                                                   int64_t npix, int pass) {
    const int b = blockIdx.y;
    const ColorOps c = load_ops(ops, factors, sums, b);
    int slot = -1, seen = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (c.op[j] == OV_COLOR_CONTRAST && seen++ == pass) slot = j;
    if (slot < 0) return;                                             // the whole block: no barrier is skipped by part of it
    const unsigned char* src = resized + (int64_t)b * npix * 3;
    unsigned long long acc = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        int r = src[3 * i], g = src[3 * i + 1], bl = src[3 * i + 2];
        apply_ops(c, slot, (double)npix, r, g, bl);
        acc += (unsigned long long)luma(r, g, bl);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&sums[4 * b + slot], part[0] + part[1] + part[2] + part[3]);
}

// the operations in order, ToTensor (x / 255), Normalize ((x - mean) / std), CHW
template <bool OUT_BF16>
__global__ __launch_bounds__(256) void tt_finish(const unsigned char* __restrict__ resized, const int* __restrict__ ops,
                                                 const float* __restrict__ factors, const unsigned long long* __restrict__ sums,
                                                 int64_t npix, float m0, float m1, float m2, float d0, float d1, float d2,
                                                 void* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= npix) return;
    const ColorOps c = load_ops(ops, factors, sums, b);
    const unsigned char* p = resized + ((int64_t)b * npix + i) * 3;
    int r = p[0], g = p[1], bl = p[2];
    apply_ops(c, 4, (double)npix, r, g, bl);
    const float v0 = ((float)r / 255.0f - m0) / d0;
    const float v1 = ((float)g / 255.0f - m1) / d1;
    const float v2 = ((float)bl / 255.0f - m2) / d2;
    const int64_t o = (int64_t)b * 3 * npix + i;
    if (OUT_BF16) {
        ov_bf16* d = (ov_bf16*)dst;
        d[o] = f32_to_bf16_bits(v0); d[npix + o] = f32_to_bf16_bits(v1); d[2 * npix + o] = f32_to_bf16_bits(v2);
    } else {
        float* d = (float*)dst;
        d[o] = v0; d[npix + o] = v1; d[2 * npix + o] = v2;
    }
}

bool plan_args_ok(int B, int out_h, int out_w, int interpolation, int max_taps_x, int max_taps_y) {
    return B > 0 && out_h > 0 && out_w > 0 && max_taps_x > 0 && max_taps_y > 0 &&
           (interpolation == OV_INTERP_BILINEAR || interpolation == OV_INTERP_BICUBIC);
}

}  // namespace

extern "C" size_t ov_train_transform_workspace_bytes(int B, int out_h, int out_w, int max_rows, int max_taps_x, int max_taps_y) {
    if (B <= 0 || out_h <= 0 || out_w <= 0 || max_rows <= 0 || max_taps_x <= 0 || max_taps_y <= 0) return 0;
    return tt_layout(B, out_h, out_w, max_rows, max_taps_x, max_taps_y).total;
}

extern "C" int ov_train_transform_plan(const int* boxes, int B, int out_h, int out_w, int interpolation, int max_taps_x, int max_taps_y,
                                       int* bounds_x, int* taps_x, int* bounds_y, int* taps_y, ov_stream_t stream) {
    if (!boxes || !bounds_x || !taps_x || !bounds_y || !taps_y) return OV_ERR_INVALID;
    if (!plan_args_ok(B, out_h, out_w, interpolation, max_taps_x, max_taps_y)) return OV_ERR_INVALID;
    return launch_plan(boxes, B, out_h, out_w, interpolation, max_taps_x, max_taps_y, bounds_x, taps_x, bounds_y, taps_y, nullptr,
                       (hipStream_t)stream);
}

extern "C" int ov_train_transform(const unsigned char* pixels, int64_t pixel_bytes, const int64_t* offsets, const int* shapes,
                                  const int* boxes, const int* ops, const float* factors, int B, int out_h, int out_w, int max_rows,
                                  int interpolation, int max_taps_x, int max_taps_y, int contrast_passes, const float* mean,
                                  const float* stdv, void* out, int out_dtype, void* workspace, size_t workspace_bytes,
                                  ov_stream_t stream) {
    if (!pixels || !offsets || !shapes || !boxes || !ops || !factors || !mean || !stdv || !out || !workspace) return OV_ERR_INVALID;
    if (!plan_args_ok(B, out_h, out_w, interpolation, max_taps_x, max_taps_y) || max_rows <= 0 || pixel_bytes <= 0) return OV_ERR_INVALID;
    if (contrast_passes < 0 || contrast_passes > 4) return OV_ERR_INVALID;
    if (out_dtype != OV_F32 && out_dtype != OV_BF16) return OV_ERR_INVALID;
    if (((uintptr_t)workspace & 15) != 0) return OV_ERR_INVALID;
    if (B > 65535 || max_rows > 65535 || out_h > 65535) return OV_ERR_UNSUPPORTED;      // grid y and z
    const TtLayout l = tt_layout(B, out_h, out_w, max_rows, max_taps_x, max_taps_y);
    if (workspace_bytes < l.total) return OV_ERR_WORKSPACE;
    char* ws = (char*)workspace;
    unsigned long long* sums = (unsigned long long*)(ws + l.sums);
    int* bounds_x = (int*)(ws + l.bounds_x);
    int* taps_x = (int*)(ws + l.taps_x);
    int* bounds_y = (int*)(ws + l.bounds_y);
    int* taps_y = (int*)(ws + l.taps_y);
    unsigned char* htmp = (unsigned char*)(ws + l.htmp);
    unsigned char* resized = (unsigned char*)(ws + l.resized);
    hipStream_t st = (hipStream_t)stream;

    const int rc = launch_plan(boxes, B, out_h, out_w, interpolation, max_taps_x, max_taps_y, bounds_x, taps_x, bounds_y, taps_y, sums, st);
    if (rc != OV_OK) return rc;
    hipLaunchKernelGGL(tt_resample_h, dim3((out_w + 255) / 256, max_rows, B), dim3(256), 0, st, pixels, pixel_bytes, offsets, shapes,
                       boxes, bounds_x, taps_x, max_taps_x, htmp, max_rows, out_w);
    OV_LAUNCH_CHECK();
    hipLaunchKernelGGL(tt_resample_v, dim3((out_w + 255) / 256, out_h, B), dim3(256), 0, st, htmp, max_rows, pixel_bytes, offsets,
                       shapes, boxes, bounds_y, taps_y, max_taps_y, resized, out_h, out_w);
    OV_LAUNCH_CHECK();
    const int64_t npix = (int64_t)out_h * out_w;
    const unsigned pix_blocks = (unsigned)((npix + 255) / 256);
    for (int pass = 0; pass < contrast_passes; ++pass) {
        hipLaunchKernelGGL(tt_luma_sum, dim3(pix_blocks < 256u ? pix_blocks : 256u, B), dim3(256), 0, st, resized, ops, factors, sums,
                           npix, pass);
        OV_LAUNCH_CHECK();
    }
    if (out_dtype == OV_BF16)
        hipLaunchKernelGGL(tt_finish<true>, dim3(pix_blocks, B), dim3(256), 0, st, resized, ops, factors, sums, npix, mean[0], mean[1],
                           mean[2], stdv[0], stdv[1], stdv[2], out);
    else
        hipLaunchKernelGGL(tt_finish<false>, dim3(pix_blocks, B), dim3(256), 0, st, resized, ops, factors, sums, npix, mean[0], mean[1],
                           mean[2], stdv[0], stdv[1], stdv[2], out);
    OV_LAUNCH_CHECK();
    return OV_OK;
}
