// tf_scan.hip -- inclusive prefix scans along the columns of a column-major table: running sums, running products and the affine
// recurrence y_i = a_i y_(i-1) + b_i.  Argument checks, the plan (tile, spine turn, launches), the work-space rule and the launcher
// over scan_kernels.h behind the entry points of include/tf_hip.h ("Prefix scans" has the contract).  Device pointers only: the unit
// takes no memory of its own -- the work space is the caller's, the descriptors travel as kernel arguments.
#include "tf_internal.h"
#include "scan_kernels.h"

namespace tfi {
namespace {

static_assert(TF_SCAN_SUM == tfk::kScanSum && TF_SCAN_PRODUCT == tfk::kScanProduct && TF_SCAN_AFFINE == tfk::kScanAffine, "the header's modes");
constexpr size_t kMaxLen = (size_t)1 << 30;
constexpr size_t kMaxWords = (size_t)1 << 35;

bool mode_ok(int mode) { return mode == tfk::kScanSum || mode == tfk::kScanProduct || mode == tfk::kScanAffine; }
size_t tile_of(int w) { return w == 1 ? (size_t)tfk::ScanGeom<1>::TILE : (size_t)tfk::ScanGeom<3>::TILE; }
size_t wave_of(int w) { return w == 1 ? (size_t)tfk::ScanGeom<1>::WAVE : (size_t)tfk::ScanGeom<3>::WAVE; }
size_t map_words(int mode, int w) { return mode == tfk::kScanAffine ? 2 * (size_t)w : (size_t)w; }
// every operand array of a call holds at most n * batch * width_out words; an affine call reads two of them
bool too_many_words(int mode, size_t n, size_t batch, int w) { return batch > kMaxWords / (n * map_words(mode, w)); }

size_t tiles_of(size_t n, int w) { return (n + tile_of(w) - 1) / tile_of(w); }
// the tile kernels take one workgroup of 256 threads per (column, tile), and a launch holds fewer than 2^32 threads.  Only columns
// above a wave's 64 K elements run there: the bound is first met at 2^24 columns of 1025 BFieldElements, 128 GiB per operand.
constexpr size_t kMaxTileBlocks = ((size_t)1 << 24) - 1;
bool too_many_tiles(size_t n, size_t batch, int w) { return n > wave_of(w) && batch > kMaxTileBlocks / tiles_of(n, w); }

// what (mode, n, batch, width_out) alone decide, for a call that is not empty
int check_shape(int mode, size_t n, size_t batch, int w) {
    if (!mode_ok(mode) || (w != 1 && w != 3)) return TF_ERR_INVALID_ARGUMENT;
    if (n > kMaxLen || too_many_words(mode, n, batch, w) || too_many_tiles(n, batch, w)) return TF_ERR_LEN_TOO_LARGE;
    return TF_OK;
}

size_t workspace_of(int mode, size_t n, size_t batch, int w) {
    const size_t tiles = tiles_of(n, w);
    return tiles <= 1 ? 0 : tiles * batch * (map_words(mode, w) + (size_t)w) * sizeof(u64);
}

unsigned capped(size_t blocks) { return (unsigned)std::min<size_t>(blocks, (size_t)device_cus() * 64); }

template <int MODE, int W, int WB>
int launch_t(tfk::ScanArgs& a, u64* work, hipStream_t s) {
    const size_t n = (size_t)a.n, batch = (size_t)a.batch;
    const dim3 threads(tfk::kScanThreads);
    if (n <= (size_t)tfk::ScanGeom<W>::WAVE) {
        const unsigned blocks = capped((batch + tfk::kScanWaves - 1) / tfk::kScanWaves);
        hipLaunchKernelGGL((tfk::scan_wave_kernel<MODE, W, WB>), dim3(blocks), threads, 0, s, a);
        HIPCHK(hipGetLastError());
        return TF_OK;
    }
    const size_t tiles = tiles_of(n, W);
    a.tiles = (long long)tiles;
    if (tiles > 1) {
        a.agg = work;
        a.start = work + tiles * batch * (size_t)tfk::ScanCarry<MODE, W>::WORDS;
        hipLaunchKernelGGL((tfk::scan_aggregate_kernel<MODE, W, WB>), dim3((unsigned)(batch * (tiles - 1))), threads, 0, s, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL((tfk::scan_spine_kernel<MODE, W>), dim3(capped(batch)), threads, 0, s, a);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL((tfk::scan_apply_kernel<MODE, W, WB>), dim3((unsigned)(batch * tiles)), threads, 0, s, a);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int launch(int mode, int w, int wb, tfk::ScanArgs& a, u64* work, hipStream_t s) {
    if (mode == tfk::kScanSum) return w == 1 ? launch_t<tfk::kScanSum, 1, 1>(a, work, s) : launch_t<tfk::kScanSum, 3, 3>(a, work, s);
    if (mode == tfk::kScanProduct) return w == 1 ? launch_t<tfk::kScanProduct, 1, 1>(a, work, s) : launch_t<tfk::kScanProduct, 3, 3>(a, work, s);
    if (w == 1) return launch_t<tfk::kScanAffine, 1, 1>(a, work, s);
    return wb == 1 ? launch_t<tfk::kScanAffine, 3, 1>(a, work, s) : launch_t<tfk::kScanAffine, 3, 3>(a, work, s);
}

}  // namespace

// In this order and before any HIP call: TF_OK for an empty call, TF_ERR_NULL_POINTER, TF_ERR_INVALID_ARGUMENT (mode, widths, a
// stride, a_len, a_sets, n_init, a short work space), TF_ERR_LEN_TOO_LARGE, then TF_ERR_NO_DEVICE.  mode == sum: `b` is the operand
// and `a` is not looked at; mode == product: `a` (a_len == n) is the operand and `b` is not looked at.
int scan_dev(int mode, const u64* a, size_t a_len, size_t a_sets, int wa, size_t stride_a, const u64* b, int wb, size_t stride_b, size_t n, size_t batch,
             const u64* init, size_t n_init, u64* out, size_t stride_out, void* d_work, size_t work_bytes, void* stream) {
    if (n == 0 || batch == 0) return TF_OK;
    const bool has_a = mode != tfk::kScanSum, has_b = mode != tfk::kScanProduct;
    const int w = has_a ? wa : wb;  // width_out: max(width_a, width_b) over the listed pairs
    const bool widths_ok = mode_ok(mode) && (w == 1 || w == 3) && (!has_b || wb == w || (mode == tfk::kScanAffine && wb == 1));
    // the work space a valid call of this shape needs (0 while the shape is not valid: the later checks name the reason)
    const size_t need = widths_ok && !check_shape(mode, n, batch, w) ? workspace_of(mode, n, batch, w) : 0;
    if ((has_a && !a) || (has_b && !b) || !out || (n_init && !init) || (need && !d_work)) return TF_ERR_NULL_POINTER;
    if (!widths_ok) return TF_ERR_INVALID_ARGUMENT;
    if (mode == tfk::kScanAffine && a_len != 1 && a_len != n) return TF_ERR_INVALID_ARGUMENT;
    // one multiplier per column, a_sets of them packed.  n == 1 makes a_len == 1 both forms: stride_a == 0, which no table has, says packed
    const bool a_packed = mode == tfk::kScanAffine && a_len == 1 && (n != 1 || stride_a == 0);
    if (a_packed && a_sets != 1 && a_sets != batch) return TF_ERR_INVALID_ARGUMENT;
    if (has_a && !a_packed && stride_a / (size_t)w < n) return TF_ERR_INVALID_ARGUMENT;
    if (has_b && stride_b / (size_t)wb < n) return TF_ERR_INVALID_ARGUMENT;
    if (stride_out / (size_t)w < n) return TF_ERR_INVALID_ARGUMENT;
    if (n_init != 0 && n_init != 1 && n_init != batch) return TF_ERR_INVALID_ARGUMENT;
    if (work_bytes < need) return TF_ERR_INVALID_ARGUMENT;
    TRY(check_shape(mode, n, batch, w));
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    tfk::ScanArgs s{};
    s.a = a, s.b = b, s.init = n_init ? init : nullptr, s.out = out;
    s.n = (long long)n, s.batch = (long long)batch, s.tiles = 1;
    if (a_packed) s.a_col = a_sets == batch && batch != 1 ? (long long)w : 0;
    else if (has_a) s.a_col = (long long)stride_a, s.a_row = w;
    s.stride_b = (long long)stride_b, s.stride_out = (long long)stride_out;
    s.init_col = n_init == batch && batch != 1 ? (long long)w : 0;
    return launch(mode, w, wb, s, static_cast<u64*>(d_work), static_cast<hipStream_t>(stream));
}

size_t scan_workspace(int mode, size_t n, size_t batch, int w) {
    if (n == 0 || batch == 0 || check_shape(mode, n, batch, w)) return 0;
    return workspace_of(mode, n, batch, w);
}

// info: elements per tile, tiles per column, tile maps per spine turn, launches, elements per wave (the one-wave-per-column form
// up to there), words per tile map
int scan_plan(int mode, size_t n, size_t batch, int w, int* info, int capacity) {
    if (n != 0 && batch != 0) {
        const int rc = check_shape(mode, n, batch, w);
        if (rc) return -rc;
    } else if (!mode_ok(mode) || (w != 1 && w != 3)) {
        return -TF_ERR_INVALID_ARGUMENT;
    }
    const size_t tiles = tiles_of(n, w);
    const int launches = n == 0 || batch == 0 ? 0 : tiles > 1 ? 3 : 1;
    const int v[6] = {(int)tile_of(w), (int)tiles, tfk::kScanSpineTurn, launches, (int)wave_of(w), (int)map_words(mode, w)};
    for (int i = 0; i < 6 && i < capacity && info; ++i) info[i] = v[i];
    return launches;
}

}  // namespace tfi
