// image_resize.hip - `Image.resize((width, height), filter)` of 8-bit RGB frames as Pillow computes it (ImagingResample, Resample.c), the
// resize magicanimate/pipelines/animation.py:174-185 passes every control frame and the source image through and
// EMOAnimationPipeline.py:688 the source image:
//   emo_image_resize : frames [n][H][W][3] -> [n][h][w][3].  Pillow's resize of 8-bit pixels is integer arithmetic: per axis a table of
//                      22-bit fixed-point coefficients (built on the host in doubles: emote_hack_amd/video_io.py resize_taps), a
//                      horizontal pass to 8-bit pixels, then a vertical pass over those.  Two plain launches:
//                        horizontal  a lane takes one output pixel: its taps are neighbouring pixels of one row, the three channels share
//                                    every coefficient, and the lanes of a wavefront walk neighbouring stretches of that row
//                        vertical    a lane takes one dword of the flat output, four neighbouring bytes of a row: with rows of a multiple
//                                    of 4 bytes they share their taps and every tap is ONE dword load; otherwise byte by byte.  Either
//                                    way the lanes of a wavefront walk neighbouring bytes of a row
//                      Both are bound by the rate of their loads, not by memory (profiles/image_resize.md).
// The intermediate image is 8-bit and rounded, as Pillow's is: the bytes are Pillow's.
#include "common.h"

#define IR_PRECISION_BITS 22      // Resample.c PRECISION_BITS = 32 - 8 - 2

// Every pass computes clip8((2^21 + sum_t pixel[first(o) + t] * coef[o][t]) >> 22) along its axis.  Every index taken from `bounds` is
// clamped to the axis before use: a bad table reads wrong pixels, never out of bounds.  Sums wrap in 32 bits (no table of resize_taps
// reaches that: sum |coef| < 2^23); the shift is arithmetic.
__device__ __forceinline__ uint32_t ir_clip8(uint32_t acc) { return (uint32_t)min(max((int32_t)acc >> IR_PRECISION_BITS, 0), 255); }

// horizontal: in [lines][W][3] -> out [lines][w][3], one output pixel per lane
__global__ __launch_bounds__(256) void image_resample_rows_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t n_pixels,
                                                                  int W, int w, const int32_t* __restrict__ bounds,
                                                                  const int32_t* __restrict__ coef, int ksize) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_pixels; p += (int64_t)gridDim.x * 256) {
    const int64_t line = p / w;
    const int o = (int)(p - line * w);
    const int first = min(max(bounds[2 * o], 0), W - 1);
    const int count = min(max(bounds[2 * o + 1], 0), min(ksize, W - first));
    const uint8_t* s = in + (line * W + first) * 3;
    const int32_t* c = coef + (int64_t)o * ksize;
    uint32_t a0 = 1u << (IR_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < count; t++) {
      const uint32_t k = (uint32_t)c[t];
      a0 += (uint32_t)s[3 * t] * k;
      a1 += (uint32_t)s[3 * t + 1] * k;
      a2 += (uint32_t)s[3 * t + 2] * k;
    }
    uint8_t* d = out + p * 3;
    d[0] = (uint8_t)ir_clip8(a0);
    d[1] = (uint8_t)ir_clip8(a1);
    d[2] = (uint8_t)ir_clip8(a2);
  }
}

// vertical: in [n][H][row] -> out [n][h][row] (row = 3 w bytes), one dword of the flat output per lane.  ROW4: row % 4 == 0 and `in`
// 4-byte aligned - a dword then lies inside one row, and so does the dword of every tap above it.
template <bool ROW4>
__global__ __launch_bounds__(256) void image_resample_cols_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int64_t total_bytes,
                                                                  int H, int h, int row, const int32_t* __restrict__ bounds,
                                                                  const int32_t* __restrict__ coef, int ksize) {
  const int64_t n_dwords = (total_bytes + 3) / 4;
  const int64_t out_frame = (int64_t)h * row, in_frame = (int64_t)H * row;
  for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < n_dwords; d += (int64_t)gridDim.x * 256) {
    const int64_t byte0 = d * 4;
    int64_t frame = byte0 / out_frame;
    const int rem = (int)(byte0 - frame * out_frame);
    int o = rem / row, i = rem - o * row;
    if constexpr (ROW4) {                                    // total_bytes % 4 == 0, i % 4 == 0, i + 3 < row
      const int first = min(max(bounds[2 * o], 0), H - 1);
      const int count = min(max(bounds[2 * o + 1], 0), min(ksize, H - first));
      const uint8_t* s = in + frame * in_frame + (int64_t)first * row + i;
      const int32_t* c = coef + (int64_t)o * ksize;
      uint32_t a0 = 1u << (IR_PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
      for (int t = 0; t < count; t++) {
        const uint32_t k = (uint32_t)c[t], px = *(const uint32_t*)(s + (int64_t)t * row);
        a0 += (px & 255u) * k;
        a1 += ((px >> 8) & 255u) * k;
        a2 += ((px >> 16) & 255u) * k;
        a3 += (px >> 24) * k;
      }
      *(uint32_t*)(out + byte0) = ir_clip8(a0) | ir_clip8(a1) << 8 | ir_clip8(a2) << 16 | ir_clip8(a3) << 24;
    } else {
      uint32_t v = 0;
#pragma unroll
      for (int b = 0; b < 4; b++) {
        if (byte0 + b < total_bytes) {
          const int first = min(max(bounds[2 * o], 0), H - 1);
          const int count = min(max(bounds[2 * o + 1], 0), min(ksize, H - first));
          const uint8_t* s = in + frame * in_frame + (int64_t)first * row + i;
          const int32_t* c = coef + (int64_t)o * ksize;
          uint32_t acc = 1u << (IR_PRECISION_BITS - 1);
          for (int t = 0; t < count; t++) acc += (uint32_t)s[(int64_t)t * row] * (uint32_t)c[t];
          v |= ir_clip8(acc) << (8 * b);
        }
        if (++i == row) {
          i = 0;
          if (++o == h) { o = 0; frame++; }
        }
      }
      if (byte0 + 4 <= total_bytes) {
        *(uint32_t*)(out + byte0) = v;
      } else {
        for (int b = 0; byte0 + b < total_bytes; b++) out[byte0 + b] = (uint8_t)(v >> (8 * b));
      }
    }
  }
}

static int ir_grid(int64_t items) {
  const int64_t g = (items + 255) / 256;
  return (int)(g < 65536 ? g : 65536);
}

static int image_resample_rows(const uint8_t* in, uint8_t* out, int64_t lines, int W, int w, const int32_t* bounds, const int32_t* coef,
                               int ksize, hipStream_t stream) {
  const int64_t n_pixels = lines * w;
  image_resample_rows_kernel<<<ir_grid(n_pixels), 256, 0, stream>>>(in, out, n_pixels, W, w, bounds, coef, ksize);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

// out 4-byte aligned (the caller checks)
static int image_resample_cols(const uint8_t* in, uint8_t* out, int n, int H, int h, int row, const int32_t* bounds, const int32_t* coef,
                               int ksize, hipStream_t stream) {
  const int64_t total = (int64_t)n * h * row;
  if (row % 4 == 0 && (uintptr_t)in % 4 == 0)
    image_resample_cols_kernel<true><<<ir_grid((total + 3) / 4), 256, 0, stream>>>(in, out, total, H, h, row, bounds, coef, ksize);
  else
    image_resample_cols_kernel<false><<<ir_grid((total + 3) / 4), 256, 0, stream>>>(in, out, total, H, h, row, bounds, coef, ksize);
  EMO_LAUNCH_CHECK();
  return EMO_OK;
}

static bool image_resize_shape_ok(int n, int H, int W, int h, int w) {
  const int64_t lim = (int64_t)1 << 31;
  return n > 0 && H > 0 && W > 0 && h > 0 && w > 0 && (int64_t)H * W * 3 < lim && (int64_t)h * w * 3 < lim && (int64_t)H * w * 3 < lim;
}

extern "C" size_t emo_image_resize_workspace_bytes(int n, int H, int W, int h, int w) {
  if (!image_resize_shape_ok(n, H, W, h, w) || W == w || H == h) return 0;      // one pass, or none, needs no intermediate image
  return (size_t)n * H * w * 3;
}

extern "C" int emo_image_resize(const uint8_t* frames, uint8_t* out, int n, int H, int W, int h, int w, const int32_t* xbounds,
                                const int32_t* xcoef, int kx, const int32_t* ybounds, const int32_t* ycoef, int ky, void* workspace,
                                size_t workspace_bytes, void* stream) {
  EMO_CHECK(frames && out, EMO_ERR_NULL, "emo_image_resize: null pointer");
  EMO_CHECK(image_resize_shape_ok(n, H, W, h, w), EMO_ERR_BAD_SHAPE,
            "emo_image_resize: n=%d %d x %d -> %d x %d (height x width; every size positive, a frame and its intermediate image below 2^31 bytes)",
            n, H, W, h, w);
  const bool horizontal = W != w, vertical = H != h;
  EMO_CHECK(!horizontal || (xbounds && xcoef), EMO_ERR_NULL, "emo_image_resize: the width changes and the horizontal tables are null");
  EMO_CHECK(!vertical || (ybounds && ycoef), EMO_ERR_NULL, "emo_image_resize: the height changes and the vertical tables are null");
  EMO_CHECK((!horizontal || kx > 0) && (!vertical || ky > 0), EMO_ERR_BAD_SHAPE, "emo_image_resize: kx=%d ky=%d", kx, ky);
  EMO_CHECK((uintptr_t)out % 4 == 0, EMO_ERR_BAD_SHAPE, "emo_image_resize: out must be 4-byte aligned");
  const size_t in_bytes = (size_t)n * H * W * 3, out_bytes = (size_t)n * h * w * 3;
  EMO_CHECK(out + out_bytes <= frames || frames + in_bytes <= out, EMO_ERR_BAD_SHAPE, "emo_image_resize: out overlaps the frames");
  const hipStream_t s = as_stream(stream);
  if (horizontal && vertical) {
    const size_t need = emo_image_resize_workspace_bytes(n, H, W, h, w);
    EMO_CHECK(workspace, EMO_ERR_NULL, "emo_image_resize: both sizes change and the workspace is null");
    EMO_CHECK(workspace_bytes >= need && (uintptr_t)workspace % 4 == 0, EMO_ERR_BAD_SHAPE,
              "emo_image_resize: the workspace holds %zu bytes, the intermediate image of %d x %d x %d x 3 takes %zu (4-byte aligned)",
              workspace_bytes, n, H, w, need);
    uint8_t* ws = (uint8_t*)workspace;
    EMO_CHECK((ws + need <= frames || frames + in_bytes <= ws) && (ws + need <= out || out + out_bytes <= ws), EMO_ERR_BAD_SHAPE,
              "emo_image_resize: the workspace overlaps the frames or out");
    const int rc = image_resample_rows(frames, ws, (int64_t)n * H, W, w, xbounds, xcoef, kx, s);
    if (rc != EMO_OK) return rc;
    return image_resample_cols(ws, out, n, H, h, 3 * w, ybounds, ycoef, ky, s);
  }
  if (horizontal) return image_resample_rows(frames, out, (int64_t)n * H, W, w, xbounds, xcoef, kx, s);
  if (vertical) return image_resample_cols(frames, out, n, H, h, 3 * w, ybounds, ycoef, ky, s);
  const hipError_t e = hipMemcpyAsync(out, frames, out_bytes, hipMemcpyDeviceToDevice, s);      // Image.resize to the same size: a copy
  EMO_CHECK(e == hipSuccess, EMO_ERR_HIP, "emo_image_resize: copy: %s", hipGetErrorString(e));
  return EMO_OK;
}
