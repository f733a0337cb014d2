// f110_maps.hip -- part of the C ABI (include/f110_hip.h) over the gfx950 kernels; see f110_common.h for the units.
#include "f110_handle.h"
#include "f110_mapgen.h"

// The compact forms of a map (f110_map.h) beside its classic tables, derived from them on the device.  They are an extra: a
// table beyond COMPACT_MAX_BYTES, or an allocation or copy that fails, leaves the slot with the classic form alone.  Cost: two
// more cell tables and the byte table of the 256-slot one (half a table plus its padding rows), for slot 0 only.
// The byte table is ROW-PADDED (f110_map.h: map_pad_rows) for `reach` = the handle's max_range in cells, which is fixed for
// the handle's life: P rows of 0 above and below every strip, so that the fast march needs no clamp of the row.  It is an
// extra of the extra: where the padded table does not fit (map_bytes_fit) the compact forms are built without it and the
// launch of the 256-slot form reads word codes.
static void build_compact(f110_handle::MapSlot &ns, int H, int W, double reach)
{
    const size_t n = ns.d_cells.size();
    if (n * sizeof(uint16_t) > COMPACT_MAX_BYTES) return;
    const int P = map_pad_rows(reach);
    const bool bytes = map_bytes_fit(H, W, P);
    const size_t n_b = bytes ? map_cells_bp(H, W, P) : 0;
    DevBuf<uint16_t> cells[N_COMPACT];
    DevBuf<uint8_t> cells_b;
    DevBuf<double> img[N_COMPACT];
    DevBuf<unsigned> counts;
    double classic[LUT_COMPACT[N_COMPACT - 1]];
    unsigned cnt[1 + N_COMPACT] = {};
    bool ok = counts.alloc(1 + N_COMPACT) == hipSuccess && hipMemset(counts.get(), 0, sizeof(cnt)) == hipSuccess &&
              hipMemcpy(classic, ns.d_lut_lds.get(), sizeof(classic), hipMemcpyDeviceToHost) == hipSuccess;
    for (int i = 0; ok && i < N_COMPACT; i++) {
        std::vector<double> v(classic, classic + LUT_COMPACT[i]);
        v.back() = -0.0; // the far marker
        ok = cells[i].alloc(n) == hipSuccess && img[i].upload(v.data(), v.size()) == hipSuccess;
    }
    if (ok) {
        hipLaunchKernelGGL(map_compact_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, ns.d_cells.get(), n,
                           cells[0].get(), cells[1].get(), counts.get());
        ok = hipGetLastError() == hipSuccess && hipMemcpy(cnt, counts.get(), sizeof(cnt), hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (ok && bytes && (ok = cells_b.alloc(n_b) == hipSuccess)) {
        hipLaunchKernelGGL(map_bytes_kernel, dim3((unsigned)((n_b + 255) / 256)), dim3(256), 0, nullptr, ns.d_cells.get(),
                           H, W, P, cells_b.get(), n_b);
        ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    if (!ok) { (void)hipGetLastError(); return; }
    for (int i = 0; i < N_COMPACT; i++) {
        ns.d_cells_c[i] = std::move(cells[i]);
        ns.d_lut_lds_c[i] = std::move(img[i]);
        ns.compact_out[i] = cnt[0] ? (double)cnt[1 + i] / (double)cnt[0] : 0.0;
    }
    ns.d_cells_b = std::move(cells_b);
    ns.pad_rows = bytes ? P : 0;
    ns.compact = true;
}

// Both pipelines end here.  `ns` holds the complete tables of the new map; until the descriptor is on the device nothing of the
// slot has changed, so a failed install leaves the slot, its descriptor and the handle's flags as they were.  Then the slot takes
// the new tables over (its old ones are freed: the pipelines synchronised the device before building), with new flags and epoch.
static int commit_map(f110_handle *h, int slot, f110_handle::MapSlot &&ns, int H, int W, double res, double ox, double oy, double oc,
                      double os, double oob)
{
    if (slot == 0) build_compact(ns, H, W, h->cfg.max_range * (1.0 / res)); // (the forms apply to a single map only; a handle that goes on to a map per env keeps slot 0's)
    MapDev &m = ns.dev;
    memset(&m, 0, sizeof(m));
    for (int i = 0; i < N_COMPACT; i++) { m.cells_c[i] = ns.d_cells_c[i].get(); m.lut_lds_c[i] = ns.d_lut_lds_c[i].get(); }
    m.cells_b = ns.d_cells_b.get(); m.cells_b_bytes = (unsigned)ns.d_cells_b.size();
    m.pad_rows = (unsigned)ns.pad_rows; m.strip_bytes_b = m.cells_b ? (unsigned)map_rows_b(H, ns.pad_rows) * 16u : 0u;
    m.cells = ns.d_cells.get(); m.cells_far = ns.d_cells_far.get(); m.lut = ns.d_lut.get(); m.lut_lds = ns.d_lut_lds.get(); m.dt = ns.d_dt.get();
    m.H = H; m.W = W; m.strip_bytes = (unsigned)map_rows_padded(H) * 16u; m.cells_bytes = (unsigned)(ns.d_cells.size() * sizeof(uint16_t));
    m.res = res; m.rinv = 1.0 / res;
    m.ox = ox; m.oy = oy; m.oc = oc; m.os = os;
    m.wres = W * res; // width * resolution (laser_models.py:79)
    m.hres = H * res;
    m.oob = oob;      // dt[-1, -1]
    m.lut_len = (unsigned)ns.d_lut.size();
    int e = 0;
    ns.pow2 = std::frexp(res, &e) == 0.5;
    ns.ident = (oc == 1.0 && os == 0.0);
    ns.used = true;
    if (!h->d_maps.get()) {
        DevBuf<MapDev> maps;
        HIP_TRY(maps.alloc(F110_MAX_MAPS));
        HIP_TRY(hipMemset(maps.get(), 0, sizeof(MapDev) * F110_MAX_MAPS));
        h->d_maps = std::move(maps);
    }
    HIP_TRY(hipMemcpy(h->d_maps.get() + slot, &m, sizeof(MapDev), hipMemcpyHostToDevice));
    h->slots[slot] = std::move(ns);
    h->ident = h->pow2 = true;
    for (const auto &u : h->slots)
        if (u.used) { h->ident = h->ident && u.ident; h->pow2 = h->pow2 && u.pow2; }
    h->has_map = h->slots[0].used;
    h->epoch++;
    return F110_OK;
}

// Builds the device map from a host fp64 distance table (and, when known, its
// exact squared form).  Cells whose value is not resolution*sqrt(integer) keep
// the escape code and are served from the fp64 table.
static int install_map(f110_handle *h, int slot, const double *dt, const uint32_t *d2_or_null, int H, int W, double res,
                       double ox, double oy, double oc, double os)
{
    const size_t n = (size_t)H * W;
    // padded table (one border cell on every side), 8-column strips: see MapDev
    const int Hp = map_rows_padded(H);
    const size_t n_tiled = map_cells(H, W);
    std::vector<uint16_t> cells(n_tiled, 0), cells_far(n_tiled, 0); // (border and padding: code 0 = LDS slot 0 = dt[-1, -1])
    // exact squared distance of every cell (ESC64: not of the form resolution*sqrt(integer))
    const uint64_t ESC64 = ~0ull;
    std::vector<uint64_t> d2v(n);
    for (size_t i = 0; i < n; i++) {
        uint64_t d2;
        if (d2_or_null) d2 = d2_or_null[i];
        else {
            double q = dt[i] / res;
            double r = std::nearbyint(q * q);
            d2 = (r >= 0 && r < 4.0e18) ? (uint64_t)r : ESC64;
            if (d2 != ESC64 && res * std::sqrt((double)d2) != dt[i]) d2 = ESC64;
        }
        d2v[i] = d2;
    }
    // Codes are RANKS among the distinct d2 values of this map (ascending), not d2 itself:
    // squared distances are sums of two squares, so the 1023 LDS slots reach d2 ~ 3 900
    // (62 cells) instead of 1 022 (32 cells) -- the middle of a 5 m wide road still hits LDS.
    std::vector<uint64_t> distinct(d2v);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    if (!distinct.empty() && distinct.back() == ESC64) distinct.pop_back();
    if (distinct.empty() || distinct.front() != 0) distinct.insert(distinct.begin(), 0); // rank 0 <-> 0.0 (parked rays)
    const size_t n_lut = std::max<size_t>(LUT_LDS, std::min<size_t>(distinct.size(), CODE_ESC)); // ranks 0..65534 are encodable
    std::vector<double> lut(n_lut, 0.0);
    for (size_t k = 0; k < n_lut && k < distinct.size(); k++) lut[k] = res * std::sqrt((double)distinct[k]);
    for (size_t i = 0; i < n; i++) {
        const size_t t = cell_elem((int)(i / W), (int)(i % W), Hp);
        size_t rank = CODE_ESC;
        if (d2v[i] != ESC64) rank = std::min<size_t>(std::lower_bound(distinct.begin(), distinct.end(), d2v[i]) - distinct.begin(), CODE_ESC);
        cells[t] = (uint16_t)cell_code((unsigned)rank);
        cells_far[t] = (uint16_t)rank;
    }
    ON_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize()); // the previous map may still be in use by enqueued steps
    f110_handle::MapSlot ns;
    HIP_TRY(ns.d_cells.upload(cells.data(), n_tiled));
    HIP_TRY(ns.d_cells_far.upload(cells_far.data(), n_tiled));
    HIP_TRY(ns.d_dt.upload(dt, n));
    HIP_TRY(ns.d_lut.upload(lut.data(), lut.size()));
    std::vector<double> lut_lds(LUT_LDS);
    lut_lds[SLOT_OOB] = dt[n - 1];    // dt[-1, -1]: what code 0 (the border: a look-up outside the map) reads
    std::copy(lut.begin(), lut.begin() + LDS_RANKS, lut_lds.begin() + 1);
    lut_lds[SLOT_FAR] = -0.0;         // the far marker (OFF_FAR cells take the second table): see MapDev
    HIP_TRY(ns.d_lut_lds.upload(lut_lds.data(), lut_lds.size()));
    return commit_map(h, slot, std::move(ns), H, W, res, ox, oy, oc, os, dt[n - 1]);
}

// ---------------------------------------------------------------- map pipeline on the device

static int check_edt_size(int H, int W, const char *who)
{
    if (H < 1 || W < 1 || H > 32768 || W > 32768) return fail(F110_E_INVALID, "%s: map size %dx%d outside 1..32768", who, H, W);
    return F110_OK;
}

// exact squared EDT of a device mask into a device table; *max_d2_dev (optional) receives the largest value
static int edt_squared_device(const uint8_t *mask_dev, int H, int W, uint32_t *d2_dev, unsigned *g_scratch, unsigned *max_d2_dev,
                              hipStream_t st)
{
    hipLaunchKernelGGL(edt_columns_kernel, dim3((W + 255) / 256), dim3(256), 0, st, mask_dev, H, W, g_scratch);
    HIP_TRY(hipGetLastError());
    const size_t lds = (size_t)W * sizeof(unsigned);
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void *)edt_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(edt_rows_kernel, dim3(H), dim3(256), lds, st, g_scratch, H, W, d2_dev, max_d2_dev);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

extern "C" int f110_edt_squared_dev(const uint8_t *mask_dev, int32_t H, int32_t W, uint32_t *d2_dev, void *stream)
{
    if (!mask_dev || !d2_dev) return fail(F110_E_INVALID, "f110_edt_squared_dev: null pointer");
    int rc = check_edt_size(H, W, "f110_edt_squared_dev");
    if (rc) return rc;
    DevBuf<unsigned> g;
    HIP_TRY(g.alloc((size_t)H * W));
    if ((rc = edt_squared_device(mask_dev, H, W, d2_dev, g.get(), nullptr, (hipStream_t)stream))) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); // the scratch is freed on return
    return F110_OK;
}

// Occupancy mask (device) -> all map tables, without leaving the GPU.  mask: nonzero = free.
static int install_map_occupancy_dev(f110_handle *h, int slot, const uint8_t *mask_dev, int H, int W, double res, double ox,
                                     double oy, double oc, double os)
{
    const size_t n = (size_t)H * W;
    const int Hp = map_rows_padded(H);
    const size_t n_tiled = map_cells(H, W);
    ON_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize()); // the previous map may still be in use by enqueued steps
    hipStream_t st = nullptr;
    DevBuf<unsigned> g, d2, maxv, bits, prefix, sums; // scratch
    HIP_TRY(g.alloc(n));
    HIP_TRY(d2.alloc(n));
    HIP_TRY(maxv.alloc(2));
    HIP_TRY(hipMemsetAsync(maxv.get(), 0, 2 * sizeof(unsigned), st));
    int rc = edt_squared_device(mask_dev, H, W, d2.get(), g.get(), maxv.get(), st);
    if (rc) return rc;
    unsigned max_d2 = 0;
    HIP_TRY(hipMemcpy(&max_d2, maxv.get(), sizeof(unsigned), hipMemcpyDeviceToHost));
    if (max_d2 == EDT_NONE) return fail(F110_E_INVALID, "f110_set_map_occupancy_dev: map has no occupied cell"); // (the slot is untouched)
    // ranks of the distinct d2 values: presence bitmap + exclusive prefix of its popcounts
    const int n_words = (int)(((size_t)max_d2 + 32) / 32);
    const int n_blocks = (n_words + SCAN_BLOCK_WORDS - 1) / SCAN_BLOCK_WORDS;
    HIP_TRY(bits.alloc((size_t)n_words));
    HIP_TRY(prefix.alloc((size_t)n_words));
    HIP_TRY(sums.alloc((size_t)n_blocks));
    HIP_TRY(hipMemsetAsync(bits.get(), 0, (size_t)n_words * sizeof(unsigned), st));
    hipLaunchKernelGGL(d2_mark_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d2.get(), n, bits.get());
    hipLaunchKernelGGL(rank_block_sums_kernel, dim3(n_blocks), dim3(256), 0, st, bits.get(), n_words, sums.get());
    hipLaunchKernelGGL(rank_scan_sums_kernel, dim3(1), dim3(64), 0, st, sums.get(), n_blocks, maxv.get() + 1);
    hipLaunchKernelGGL(rank_word_prefix_kernel, dim3(n_blocks), dim3(256), 0, st, bits.get(), n_words, sums.get(), prefix.get());
    HIP_TRY(hipGetLastError());
    // the new map's tables
    f110_handle::MapSlot ns;
    HIP_TRY(ns.d_cells.alloc(n_tiled));
    HIP_TRY(ns.d_cells_far.alloc(n_tiled));
    HIP_TRY(ns.d_dt.alloc(n));
    const unsigned n_lut = CODE_ESC; // ranks 0..65534 are encodable; unused slots stay 0.0
    HIP_TRY(ns.d_lut.alloc(n_lut));
    HIP_TRY(hipMemsetAsync(ns.d_lut.get(), 0, (size_t)n_lut * sizeof(double), st));
    hipLaunchKernelGGL(map_fill_border_kernel, dim3((unsigned)((n_tiled + 255) / 256)), dim3(256), 0, st, ns.d_cells.get(), ns.d_cells_far.get(), n_tiled);
    hipLaunchKernelGGL(map_encode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d2.get(), H, W, Hp, bits.get(), prefix.get(), res,
                       ns.d_cells.get(), ns.d_cells_far.get(), ns.d_dt.get());
    hipLaunchKernelGGL(map_lut_kernel, dim3((n_words + 255) / 256), dim3(256), 0, st, bits.get(), n_words, prefix.get(), res, ns.d_lut.get(), n_lut);
    HIP_TRY(hipGetLastError());
    // LDS image of the LUT: its first slots, with the two special ones (see MapDev)
    std::vector<double> lut_lds(LUT_LDS);
    double oob = 0;
    HIP_TRY(hipMemcpy(lut_lds.data() + 1, ns.d_lut.get(), LDS_RANKS * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&oob, ns.d_dt.get() + (n - 1), sizeof(double), hipMemcpyDeviceToHost));
    lut_lds[SLOT_OOB] = oob;
    lut_lds[SLOT_FAR] = -0.0;
    HIP_TRY(ns.d_lut_lds.upload(lut_lds.data(), lut_lds.size()));
    return commit_map(h, slot, std::move(ns), H, W, res, ox, oy, oc, os, oob);
}


extern "C" int f110_track_mask(const double *pts_dev, int32_t n_pts, int32_t closed, int32_t H, int32_t W, double x0, double y0,
                               double pixel, double offset, double half_stroke, uint8_t *mask_dev, void *stream)
{
    if (!pts_dev || !mask_dev) return fail(F110_E_INVALID, "f110_track_mask: null pointer");
    if (n_pts < 2 || H < 1 || W < 1 || H > 32768 || W > 32768 || !(pixel > 0) || !(half_stroke >= 0))
        return fail(F110_E_INVALID, "f110_track_mask: bad arguments (n_pts=%d, %dx%d, pixel=%g)", n_pts, H, W, pixel);
    hipLaunchKernelGGL(track_mask_kernel, dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, (hipStream_t)stream, pts_dev, n_pts,
                       closed ? 1 : 0, H, W, x0, y0, pixel, offset, half_stroke, mask_dev);
    HIP_TRY(hipGetLastError());
    return F110_OK;
}

static int check_map_args(f110_handle *h, const void *p, int H, int W, double res, const char *who)
{
    if (!h || !p) return fail(F110_E_INVALID, "%s: null argument", who);
    if (H < 1 || W < 1 || (int64_t)(H + 10) * (W + 10) > (int64_t)1 << 30 || H + 10 >= (1 << 20)) return fail(F110_E_INVALID, "%s: bad map size %dx%d", who, H, W);
    // cell_offset and the march loops multiply (c >> 3) by strip_bytes - 16 as signed 24-bit operands (v_mad_i32_i24); the
    // byte table's (c >> 4) by the same strip_bytes - 16
    if (16 * (int64_t)map_rows_padded(H) - 16 >= (int64_t)1 << 23 || (W >> 3) >= (1 << 23) || (W >> 4) >= (1 << 23))
        return fail(F110_E_INVALID, "%s: map size %dx%d outside the 24-bit strip addressing (height <= 524286, width < 2^26)", who, H, W);
    if (!(res > 0) || !std::isfinite(res)) return fail(F110_E_INVALID, "%s: bad resolution %g", who, res);
    return F110_OK;
}

static int check_slot(f110_handle *h, int slot, const char *who)
{
    if (!h) return fail(F110_E_INVALID, "%s: null handle", who);
    if (slot < 0 || slot >= F110_MAX_MAPS) return fail(F110_E_INDEX, "%s: map slot %d outside 0..%d", who, slot, F110_MAX_MAPS - 1);
    return F110_OK;
}

extern "C" int f110_set_map_slot_occupancy(f110_handle *h, int32_t slot, const uint8_t *mask, int32_t H, int32_t W, double res,
                                           double ox, double oy, double oc, double os)
{
    int rc = check_slot(h, slot, "f110_set_map_slot_occupancy");
    if (rc || (rc = check_map_args(h, mask, H, W, res, "f110_set_map_occupancy")) || (rc = check_edt_size(H, W, "f110_set_map_occupancy")))
        return rc;
    const size_t n = (size_t)H * W;
    if (!memchr(mask, 0, n)) return fail(F110_E_INVALID, "f110_set_map_occupancy: map has no occupied cell");
    ON_DEVICE(h->cfg.device);
    DevBuf<uint8_t> mask_dev;
    HIP_TRY(mask_dev.upload(mask, n));
    return install_map_occupancy_dev(h, slot, mask_dev.get(), H, W, res, ox, oy, oc, os);
}

extern "C" int f110_set_map_slot_occupancy_dev(f110_handle *h, int32_t slot, const uint8_t *mask_dev, int32_t H, int32_t W,
                                               double res, double ox, double oy, double oc, double os)
{
    int rc = check_slot(h, slot, "f110_set_map_slot_occupancy_dev");
    if (rc || (rc = check_map_args(h, mask_dev, H, W, res, "f110_set_map_occupancy_dev")) ||
        (rc = check_edt_size(H, W, "f110_set_map_occupancy_dev")))
        return rc;
    return install_map_occupancy_dev(h, slot, mask_dev, H, W, res, ox, oy, oc, os);
}

extern "C" int f110_set_map_occupancy(f110_handle *h, const uint8_t *mask, int32_t H, int32_t W, double res,
                                      double ox, double oy, double oc, double os)
{
    return f110_set_map_slot_occupancy(h, 0, mask, H, W, res, ox, oy, oc, os);
}

extern "C" int f110_set_map_occupancy_dev(f110_handle *h, const uint8_t *mask_dev, int32_t H, int32_t W, double res,
                                          double ox, double oy, double oc, double os)
{
    return f110_set_map_slot_occupancy_dev(h, 0, mask_dev, H, W, res, ox, oy, oc, os);
}

extern "C" int f110_set_map_dt(f110_handle *h, const double *dt, int32_t H, int32_t W, double res, double ox,
                               double oy, double oc, double os)
{
    int rc = check_map_args(h, dt, H, W, res, "f110_set_map_dt");
    if (rc) return rc;
    return install_map(h, 0, dt, nullptr, H, W, res, ox, oy, oc, os);
}

extern "C" int f110_get_map_slot_dt(f110_handle *h, int32_t slot, double *out)
{
    int rc = check_slot(h, slot, "f110_get_map_slot_dt");
    if (rc) return rc;
    if (!out) return fail(F110_E_INVALID, "f110_get_map_slot_dt: null argument");
    const f110_handle::MapSlot &sl = h->slots[slot];
    if (!sl.used) return fail(F110_E_NOMAP, "Map is not set for scan simulator.");
    ON_DEVICE(h->cfg.device);
    HIP_TRY(hipMemcpy(out, sl.d_dt.get(), (size_t)sl.dev.H * sl.dev.W * sizeof(double), hipMemcpyDeviceToHost));
    return F110_OK;
}

extern "C" int f110_get_map_dt(f110_handle *h, double *out) { return f110_get_map_slot_dt(h, 0, out); }

// env -> map slot.  The SCAN_WAVES consecutive cars of a scan workgroup share the LDS copy of their map's LUT; where
// that holds for every workgroup (maps in blocks of envs whose car count is a multiple of SCAN_WAVES) the scan keeps that
// shape.  Otherwise -- a map per env, odd blocks -- it runs one wave per workgroup, each staging its own car's LUT:
// same results, fewer waves per CU (the LDS copies then cap a CU at 19 waves instead of 32).
extern "C" int f110_assign_maps(f110_handle *h, const int32_t *map_of_env)
{
    if (!h) return fail(F110_E_INVALID, "f110_assign_maps: null handle");
    const int B = h->cfg.num_envs, A = h->cfg.num_agents, N = B * A;
    std::vector<int32_t> m(B, 0);
    bool multi = false, single = false;
    if (map_of_env)
        for (int e = 0; e < B; e++) {
            const int k = map_of_env[e];
            if (k < 0 || k >= F110_MAX_MAPS || !h->slots[k].used)
                return fail(F110_E_INDEX, "f110_assign_maps: env %d uses map slot %d, which holds no map", e, k);
            m[e] = k;
            multi = multi || k != 0;
        }
    if (multi)
        for (int c = 0; c < N && !single; c += SCAN_WAVES)
            for (int j = 1; j < SCAN_WAVES && c + j < N; j++)
                if (m[(c + j) / A] != m[c / A]) { single = true; break; }
    ON_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize()); // enqueued steps may still read the table
    HIP_TRY(h->d_env_map.upload(m.data(), B));
    h->h_env_map = m;
    h->multi = multi;
    h->wg_single = single;
    h->epoch++;
    return F110_OK;
}
