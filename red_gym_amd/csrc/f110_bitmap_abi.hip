// f110_bitmap_abi.hip -- part of the C ABI (include/f110_hip.h) over the gfx950 kernels; see f110_common.h for the units.
#include "f110_common.h"
#include "f110_bitmap.h"

// ---------------------------------------------------------------- scan -> bitmap
static const void *bitmap_fn(size_t lds, int mode, int channels)
{
    if (bm_fetch_ahead(mode, channels)) return (const void *)&bitmap_kernel<6, true>; // (its LDS leaves room for three workgroups per CU at most)
    return bm_waves_per_eu(lds) == 8 ? (const void *)&bitmap_kernel<8, false> : (const void *)&bitmap_kernel<6, false>;
}

struct f110_bitmap {
    f110_bitmap_config cfg;
    DevBuf<int32_t> d_idx;
    DevBuf<double> d_cos, d_sin;
    int S = 0;
    size_t lds[2] = {0, 0};  // dynamic LDS of a launch on fp32 / fp64 scans (the ranges' staging buffers differ)
    int resident[2] = {0, 0}; // workgroups of bitmap_kernel the device runs at once (the launch's grid: a workgroup loops over images)
};

extern "C" void f110_bitmap_destroy(f110_bitmap *b)
{
    if (!b) return;
    DeviceScope on_dev(b->cfg.device);
    delete b;
}

extern "C" int f110_bitmap_create(const f110_bitmap_config *cfg, const int32_t *indices, const double *cosines,
                                  const double *sines, f110_bitmap **out)
{
    if (!cfg || !indices || !cosines || !sines || !out) return fail(F110_E_INVALID, "f110_bitmap_create: null argument");
    const int T = cfg->target_beam_count;
    // the reference's assertions (lidar.py:50-56)
    if (!(T > 0 && T < cfg->num_beams)) return fail(F110_E_INVALID, "target_beam_count must satisfy 0 < %d < len(scan) = %d", T, cfg->num_beams);
    if (T > 2048) return fail(F110_E_INVALID, "target_beam_count %d > 2048", T);
    if (cfg->num_beams > 65536) return fail(F110_E_INVALID, "scans of more than 65536 beams are not supported (%d)", cfg->num_beams);
    if (cfg->rows <= 0 || cfg->cols <= 0) return fail(F110_E_INVALID, "output_image_dims must be at least 1x1");
    if (cfg->rows > 4096 || cfg->cols > 4096) return fail(F110_E_INVALID, "output_image_dims above 4096 are not supported");
    if (cfg->channels != 1 && cfg->channels != 3 && cfg->channels != 4) return fail(F110_E_INVALID, "channels must 1, 3, or 4");
    if (cfg->draw_mode < F110_BITMAP_FILL || cfg->draw_mode > F110_BITMAP_RAYS) return fail(F110_E_INVALID, "draw_mode must be FILL, POLYGON or RAYS");
    for (int k = 0; k < T; k++)
        if (indices[k] < 0 || indices[k] >= cfg->num_beams) return fail(F110_E_INDEX, "beam index %d out of range", indices[k]);
    int S = (cfg->cols + 31) / 32;
    S |= 1; // odd row pitch: the per-row parity pass is LDS-bank-conflict free
    const size_t lds = bitmap_lds_bytes(T, cfg->rows, S, cfg->draw_mode, cfg->channels, 1); // (fp64 scans: the larger of the two layouts)
    if (lds > 150 * 1024) return fail(F110_E_INVALID, "image %dx%d with %d beams needs %zu bytes of LDS (limit 150 KiB)", cfg->rows, cfg->cols, T, lds);
    f110_bitmap *b = new (std::nothrow) f110_bitmap;
    if (!b) return fail(F110_E_INVALID, "out of memory");
    b->cfg = *cfg; b->S = S; b->lds[1] = lds; b->lds[0] = bitmap_lds_bytes(T, cfg->rows, S, cfg->draw_mode, cfg->channels, 0);
    DeviceScope on_dev(cfg->device);
    if (on_dev.err != hipSuccess) { delete b; return fail(F110_E_HIP, "hipSetDevice(%d) failed", cfg->device); }
    hipError_t e = b->d_idx.upload(indices, T);
    if (e == hipSuccess) e = b->d_cos.upload(cosines, T);
    if (e == hipSuccess) e = b->d_sin.upload(sines, T);
    if (e == hipSuccess && lds > 64 * 1024)
        e = hipFuncSetAttribute(bitmap_fn(lds, cfg->draw_mode, cfg->channels), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) {
        int dev = 0;
        hipDeviceProp_t prop;
        e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipGetDeviceProperties(&prop, dev);
        for (int f = 0; f < 2 && e == hipSuccess; f++) {
            int per_cu = 0;
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bitmap_fn(b->lds[f], cfg->draw_mode, cfg->channels), BM_THREADS, b->lds[f]);
            b->resident[f] = std::max(1, per_cu) * std::max(1, prop.multiProcessorCount);
        }
    }
    if (e != hipSuccess) { f110_bitmap_destroy(b); return fail(F110_E_HIP, "f110_bitmap_create: %s", hipGetErrorString(e)); }
    *out = b;
    return F110_OK;
}

// f110_bitmap_render and f110_bitmap_render_bits (`who`): exactly one of `out` / `out_bits` is the launch's output
static int bitmap_launch(const char *who, f110_bitmap *b, const void *scans, int32_t scans_f64, int64_t n, int64_t stride,
                         uint8_t *out, uint64_t *out_bits, void *stream)
{
    if (!b || n < 0) return fail(F110_E_INVALID, "%s: bad arguments", who);
    if (n == 0) return F110_OK;
    if (!scans || (!out && !out_bits)) return fail(F110_E_INVALID, "%s: null pointer", who);
    if (stride < b->cfg.num_beams || n > 0x7fffffff) return fail(F110_E_INVALID, "%s: stride %lld < num_beams or n too large", who, (long long)stride);
    if (((uintptr_t)out | (uintptr_t)out_bits) % 16) return fail(F110_E_INVALID, "%s: out must be 16-byte aligned", who);
    if (int rc = check_current_device(b->cfg.device, who)) return rc;
    BitmapArgs a;
    a.scans = scans; a.is_f64 = scans_f64 != 0; a.stride = stride; a.n = (int)n;
    a.idx = b->d_idx.get(); a.cosv = b->d_cos.get(); a.sinv = b->d_sin.get(); a.T = b->cfg.target_beam_count;
    a.rows = b->cfg.rows; a.cols = b->cfg.cols; a.channels = b->cfg.channels; a.mode = b->cfg.draw_mode;
    a.bg = b->cfg.bg_value; a.draw = b->cfg.draw_value; a.draw_center = b->cfg.draw_center;
    a.scale = b->cfg.scaling_factor; a.out = out; a.out_bits = (unsigned long long *)out_bits; a.S = b->S; a.qcap = bm_queue_cap(a.T, a.mode);
    const char *grid_env = getenv("F110_BM_GRID"); // test hook (test_gpu_bitmap.py): workgroups of the launch (read per call)
    // fetch-ahead shape: as many workgroups as the device runs at once, each looping over images; else one per image
    const int64_t grid = !bm_fetch_ahead(a.mode, a.channels) ? n : std::min<int64_t>(n, grid_env && atoi(grid_env) > 0 ? atoi(grid_env) : b->resident[a.is_f64]);
    void *params[1] = {(void *)&a};
    HIP_TRY(hipLaunchKernel(bitmap_fn(b->lds[a.is_f64], a.mode, a.channels), dim3((unsigned)grid), dim3(BM_THREADS), params, b->lds[a.is_f64], (hipStream_t)stream));
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_bitmap_render(f110_bitmap *b, const void *scans, int32_t scans_f64, int64_t n, int64_t stride,
                                  uint8_t *out, void *stream)
{
    return bitmap_launch("f110_bitmap_render", b, scans, scans_f64, n, stride, out, nullptr, stream);
}

extern "C" int f110_bitmap_render_bits(f110_bitmap *b, const void *scans, int32_t scans_f64, int64_t n, int64_t stride,
                                       uint64_t *out, void *stream)
{
    return bitmap_launch("f110_bitmap_render_bits", b, scans, scans_f64, n, stride, nullptr, out, stream);
}

extern "C" int f110_bitmap_points(f110_bitmap *b, const void *scans, int32_t scans_f64, int64_t n, int64_t stride,
                                  int32_t *points, void *stream)
{
    if (!b || n < 0) return fail(F110_E_INVALID, "f110_bitmap_points: bad arguments");
    if (n == 0) return F110_OK;
    if (!scans || !points) return fail(F110_E_INVALID, "f110_bitmap_points: null pointer");
    if (stride < b->cfg.num_beams || n > 0x7fffffff) return fail(F110_E_INVALID, "f110_bitmap_points: stride %lld < num_beams or n too large", (long long)stride);
    if (int rc = check_current_device(b->cfg.device, "f110_bitmap_points")) return rc;
    BitmapArgs a;
    memset(&a, 0, sizeof(a));
    a.scans = scans; a.is_f64 = scans_f64 != 0; a.stride = stride; a.n = (int)n;
    a.idx = b->d_idx.get(); a.cosv = b->d_cos.get(); a.sinv = b->d_sin.get(); a.T = b->cfg.target_beam_count;
    a.rows = b->cfg.rows; a.cols = b->cfg.cols; a.scale = b->cfg.scaling_factor;
    const long long items = (long long)n * a.T;
    hipLaunchKernelGGL(bitmap_points_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, points);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_scan_occupancy(const void *scans, int32_t scans_f64, int64_t n, int64_t stride, int32_t num_beams,
                                   const double *cosines, const double *sines, double max_range, double lo, double hi,
                                   int32_t grid, uint8_t *out, void *stream)
{
    if (n < 0 || num_beams <= 0 || grid <= 0 || grid > 1024) return fail(F110_E_INVALID, "f110_scan_occupancy: bad arguments");
    if (n == 0) return F110_OK;
    if (!scans || !cosines || !sines || !out) return fail(F110_E_INVALID, "f110_scan_occupancy: null pointer");
    if (stride < num_beams || n > 0x7fffffff) return fail(F110_E_INVALID, "f110_scan_occupancy: stride < num_beams or n too large");
    if ((uintptr_t)out % 16) return fail(F110_E_INVALID, "f110_scan_occupancy: out must be 16-byte aligned");
    OccArgs a;
    a.scans = scans; a.is_f64 = scans_f64 != 0; a.stride = stride; a.n = (int)n; a.num_beams = num_beams;
    a.cosv = cosines; a.sinv = sines; a.max_range = max_range; a.lo = lo; a.hi = hi; a.grid = grid; a.out = out;
    const size_t lds = (size_t)((grid * grid + 31) / 32) * 4;
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)occupancy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(occupancy_kernel, dim3((unsigned)n), dim3(BM_THREADS), lds, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}
