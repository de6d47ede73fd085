// tf_plan.hip -- the NTT planner of libtf_hip.so: which route a transform call takes and, for a multi-pass plan, its passes,
// radices, tile batch and tile streams (ntt_plan.h).  Host logic only: no kernel lives here, nothing is launched, no device
// context is touched -- run_ntt (tf_ntt.hip) executes what plan_ntt decides, and the introspection calls of the ABI read the same
// plan.  Every threshold sits next to the measurement it comes from; the tf_set_ntt_* mode words live here with their rules.
#include "tf_internal.h"

namespace tfi {

int ilog2(size_t v) {
    int l = 0;
    while ((size_t(1) << l) < v) ++l;
    return l;
}

// ------------------------------------------------------------------------------------ deployment settings
size_t g_tile_bytes = 0;
// Pipelined tiles: with g_pipe = K > 1 the batch tiles of a multi-pass transform are dealt round-robin to K side streams,
// each with its own scratch tile, so that the column pass of tile t + 1 runs beside the transposing pass of tile t: the
// launches' tails fill each other and a tile sized for the 256 MiB Infinity Cache is re-read out of it.  1 = one stream.
std::atomic<int> g_pipe{0};
std::once_flag g_env_once;
void read_env() {
    std::call_once(g_env_once, [] {
        if (g_tile_bytes == 0) {
            const char* s = getenv("TF_NTT_TILE_BYTES");
            g_tile_bytes = s ? strtoull(s, nullptr, 10) : (size_t(2048) << 20);
            if (g_tile_bytes == 0) g_tile_bytes = size_t(2048) << 20;
        }
        if (g_pipe.load() == 0) {  // 0 = automatic (plan_ntt decides by plan); TF_NTT_PIPE / tf_set_ntt_pipe pin it
            const char* s = getenv("TF_NTT_PIPE");
            if (s && atoi(s) > 0) g_pipe.store(std::min(atoi(s), kMaxPipe));
        }
    });
}

// ------------------------------------------------------------------------------------ test hooks
std::atomic<int> g_min_passes{0};          // tf_set_ntt_min_passes
std::atomic<int> g_lat_mode{-1};           // tf_set_ntt_latency_kernel: -1 automatic, 0 never, 1 whenever the shape allows
std::atomic<int> g_pre2_mode{-1};          // tf_set_ntt_two_pass: -1 automatic, 0 never, 1 or 2 whenever supported (pairs), 3 (one-workgroup first pass)
std::atomic<int> g_small_launch_mode{-1};  // tf_set_ntt_small_launch: -1 automatic, 0 never, 1 always (tests)

// ------------------------------------------------------------------------------------ workgroup geometry
// Workgroup geometry:
//   512 threads: 16 columns per tile (128-byte segments), 64 KiB exchange rounds, 2 workgroups per CU;
//   256 threads:  8 columns per tile (64-byte segments, adjacent tiles paired on one XCD), 32 KiB rounds, 4 per CU.
// A call with too little work to fill the chip with 512-thread tiles (a single slice of <= 2^20 points: 64 tiles for 256 CUs) is
// planned with 256-thread workgroups and the generic last pass instead -- twice as many tiles of half the width: 2^16 44 -> 37 us,
// 2^18 47.5 -> 39.7, 2^20 51.8 -> 43.8 us per call; from 2^22 words per call on the wide tiles win (tools/small_batch.py).
// plan_ntt decides per call (NttPlan::wg, NttPlan::narrow) and the width travels with the plan.

// Whether a multi-pass call is planned with the narrow (256-thread) tiles: too little work to fill the chip with 512-thread ones;
// a truncating call keeps the R = 1024 last pass its caller planned for.
static bool small_launch_for(const NttShape& s) {
    const int small_mode = g_small_launch_mode.load(std::memory_order_relaxed);
    const bool small_call = (unsigned long long)s.n * s.cosets * s.batch * s.L <= (1ull << 21);
    return s.n_out < 0 && (small_mode == 1 || (small_mode < 0 && small_call));
}

// ------------------------------------------------------------------------------------ the latency-shaped kernels
// When: the call holds too little work to fill the chip with 32-element threads (measured crossover, tools/lat_sweep.py).
bool lat_wanted(int log_n, size_t batch, int L) {
    // measured crossover against the pass / block kernels (tools/lat_sweep.py, profiles/r03_lat_sweep_*.txt): 2.0 - 2.9 x faster up
    // to 2^20 words per call, level at 2^22 words (BFieldElement) / 1.5 x 2^20 words (XFieldElement: its loads step 24 bytes)
    const long long limit = L == 1 ? (1ll << 22) : (3ll << 19);
    const int mode = g_lat_mode.load(std::memory_order_relaxed);
    if (mode == 0) return false;
    if (log_n < 6 || log_n > 12) return false;
    if (mode == 1) return true;
    return (long long)(batch * size_t(L)) << log_n <= limit;
}
bool lat2_wanted(int log_n, size_t batch, int L) {
    const int mode = g_lat_mode.load(std::memory_order_relaxed);
    if (mode == 0) return false;
    if (log_n < 13 || log_n > 20) return false;
    if (mode == 1) return true;
    // measured crossover against the pass / block kernels, words per call (tools/lat_sweep.py 13 20, profiles/r03_lat2_sweep_*.txt):
    // one 2^16-point slice 33 -> 16 us; the win ends where the chip fills, and earlier for the longest lines (a 1024-point line
    // leaves two lines per workgroup: 16-byte segments)
    static const long long lim1[8] = {1ll << 21, 1ll << 21, 1ll << 21, 1ll << 21, 1ll << 21, 1ll << 20, 1ll << 20, 1ll << 20};  // log_n = 13 .. 20
    static const long long lim3[8] = {3ll << 20, 3ll << 20, 3ll << 19, 3ll << 20, 3ll << 19, 3ll << 18, 0, 0};
    const long long limit = (L == 1 ? lim1 : lim3)[log_n - 13];
    return (long long)(batch * size_t(L)) << log_n <= limit;
}

// ------------------------------------------------------------------------------------ passes and radices
int pass_count(int log_n) {  // global passes of a transform with log_n > 10
    int P = log_n <= 20 ? 2 : (log_n <= 30 ? 3 : 4);
    const int want = g_min_passes.load(std::memory_order_relaxed);  // test hook: deeper plans at small sizes
    if (want > P && want <= 4 && log_n >= 5 * want) P = want;
    return P;
}

// Radix split of a multi-pass plan: a[0..P-1], sum = log_n, every a[i] in [5, 10].
void choose_split(int log_n, int P, int L, int (&a)[4]) {
    // The last pass gets the largest radix it can (R = 1024 whenever possible: the specialised kernel with constant P2
    // and stores fused into level 5, 128-byte output segments); the column passes share the rest evenly, larger first.
    // Measured against the even split (2^28 words per call): 2^15 1.92 vs 2.62 ms, 2^18 2.20 vs 2.48,
    // 2^22 3.18 vs 3.49, 2^24 3.31 vs 4.15, 2^26 3.58 vs 3.99.
    // XFieldElement slices (L = 3) follow the same rule for n = 2^15, 2^20 and n >= 2^23 now that the R = 1024 kernel tiles
    // their rows by whole 128-byte lines (a sweep of the last radix: 2^15 1.62 vs 1.83 ms, 2^23 2.62 vs 2.71, 2^25 2.71 vs 2.86 per
    // 3 * 2^26 words); the sweep still prefers R = 32 for n < 2^15 and R = 512 for 2^16 .. 2^19 (all within 1 % of R = 1024).
    int last = std::min(10, log_n - 5 * (P - 1));
    // (round 5, profiles/r05_xfe_split2_sweep.txt: 2^13 has no better split than (8, 5) -- 1.61 ms against 1.61-1.75 for every other --
    // it is simply the first length that no longer fits one workgroup's LDS; 2^14 prefers (5, 9): 1.325 vs 1.367 ms)
    if (L == 3 && P == 2 && log_n < 20 && log_n != 15) last = log_n < 14 ? 5 : 9;
    a[P - 1] = last;
    int rest = log_n - last;
    if (P == 3 && last == 10 && log_n <= (L == 3 ? 25 : 23)) {
        // (log_n - 15, 5, 10): an exchange-free radix-32 pass in the middle (XFE 2^21 2.26 vs 2.33 ms,
        // 2^23 2.34 vs 2.45, 2^25 2.49 vs 2.51 per 3 * 2^26 words; BFE 2^22 2.90 vs 3.04, 2^23 3.01 vs 3.09 per 2^28)
        a[1] = 5;
        a[0] = rest - 5;
        // BFieldElement 2^21 / 2^22: the radix-32 pass first, (5, log_n - 15, 10) -- since the column passes run lazy networks
        // through buffer addressing (COL) the order matters only there: 2^21 2.49 vs 2.71 ms, 2^22 2.54 vs 2.59 ms per 2^28
        // words; from 2^23 on and for XFieldElement slices both orders measure the same
        if (L == 1 && log_n <= 22) a[0] = 5, a[1] = rest - 5;
    } else {
        for (int i = 0; i + 1 < P; ++i) {
            a[i] = (rest + (P - 1 - i) - 1) / (P - 1 - i);
            rest -= a[i];
        }
    }
}

// Two-pass plans for 2^21 / 2^22 points (a 2048-point pass = pairs of 1024-point workgroups, ntt_kernels.h PRE2).  Plain
// transforms, coset evaluation (forward) and coset interpolation (inverse), on the wide tiles only (g: the call's geometry).
static bool pre2_plan_ok(const NttShape& s, int log_n, const NttPlan& g) {
    const int mode = g_pre2_mode.load(std::memory_order_relaxed);
    if (mode == 0) return false;
    if (log_n < 21 || log_n > 22 || s.cosets != 1 || s.in2 || s.n_out >= 0) return false;
    const bool load_work = s.pre_scale || s.n_coeffs >= 0;
    if ((load_work && s.inverse) || (s.post_scale && !s.inverse)) return false;      // shapes no caller produces
    if (g.narrow || g.wg != 512) return false;  // (the narrow tiles take the generic last pass, not LAST1024)
    if (g_min_passes.load(std::memory_order_relaxed) > 2) return false;
    return (unsigned long long)s.n * s.L * 8 + (1ull << 20) < (1ull << 32);          // buffer addressing (fits_buffer_offsets)
}
// Round 6: the FIRST pass of a two-pass plan as ONE workgroup per 2048 x 8 tile (ntt_col2048_kernel): every element is loaded (and,
// in a coset evaluation, scaled) once, where a PRE2 pair does both twice.  2^22 = 2048 (this kernel) x 2048 (the PRE2 last pass);
// 2^21 = 2048 (this kernel) x 1024 (the plain R = 1024 last pass, no pair anywhere).  MEASURED (profiles/r06_c4_cols8_ab.txt, same
// process, same words, ms per 2^28 / 3 * 2^26 words): it wins where the first pass SCALES, at 2^22 -- XFE coset evaluation 1.84 vs 1.94
// (BASELINE configs[3]: 7.40 vs 7.80), BFE 2.53 vs 2.65 -- ties on BFE 2^21 / 2^22 plain transforms and loses 2-9 % on XFE plain
// transforms and everything XFE at 2^21 (its 64-byte segments cost more there than the pair's second read).  So the automatic plan
// takes it for coset evaluations of 2^22 points only; tf_set_ntt_two_pass(3) forces it wherever the two-pass plan applies, (1) forces
// the round-3 pairs.
static bool c8_first_pass(int log_n, bool scaled) {
    const int mode = g_pre2_mode.load(std::memory_order_relaxed);
    if (mode == 3) return true;
    if (mode >= 0) return false;
    return log_n == 22 && scaled;
}
static void pre2_split(int log_n, int (&a)[4], bool c8) {
    // 2^21: the 2048-point pass last (the first pass of a coset evaluation then scales every coefficient once); 2^22: both
    a[0] = log_n == 22 ? 11 : 10, a[1] = 11, a[2] = a[3] = 0;
    if (c8) a[0] = 11, a[1] = log_n - 11;
}

// ------------------------------------------------------------------------------------ the plan of one call
// The one route ladder.  large: the latency-shaped kernels and the narrow tiles are ruled out (plan_ntt_large).
static NttPlan plan_call(const NttShape& s, bool large) {
    NttPlan p;
    read_env();
    const int log_n = ilog2(s.n);
    const int min_passes = g_min_passes.load(std::memory_order_relaxed);
    const bool load_work = s.pre_scale || s.n_coeffs >= 0;
    p.wg = 512;  // (every route but Passes runs on the wide geometry, the single-pass Row route included)
    const auto take = [&p](NttRoute route, size_t launches) {
        p.route = route;
        p.launches = (int)launches;
        return p;
    };
    // batches of short contiguous transforms: wave-private tiles, one coalesced round trip (a handful of them stay on the tiny kernel)
    if (log_n >= 1 && (log_n <= 5 || (log_n == 6 && s.L == 1)) && !load_work && !s.post_scale && !s.in2 && s.n_out < 0 && s.packed &&
        (log_n == 5 || (s.batch << log_n) * size_t(s.L) >= 4096))
        return take(NttRoute::Rows32, 1);  // (a grid-stride walk: one launch whatever the batch)
    if (log_n <= 4) return take(NttRoute::Tiny, 1);
    // (the latency-shaped kernel also takes the coset scalings of fast_coset_evaluate / fast_coset_interpolate: a 2^10-point coset
    //  evaluation is one launch of 8-element threads, 8 us, instead of one 32-element-thread workgroup, 19 us)
    if (!large && s.n_out < 0 && s.cosets == 1 && (!s.in2 || s.L == 1) && min_passes == 0 && !(s.pre_scale && s.inverse) &&
        !(s.post_scale && !s.inverse)) {
        if (lat_wanted(log_n, s.batch, s.L)) return take(NttRoute::Lat, (s.batch + (size_t(1) << 22) - 1) >> 22);  // 2^31 threads per launch
        if (lat2_wanted(log_n, s.batch, s.L)) return take(NttRoute::Lat2, 2);                                      // column pass + last pass
    }
    if (log_n <= 10) return take(NttRoute::Row, (s.batch + (size_t(1) << 24) - 1) >> 24);  // 2^31 columns per launch
    {
        const bool product_inverse = s.in2 && s.inverse && !load_work && !s.post_scale;
        // XFieldElement slices take the same kernel as three limb transforms per slice with element stride 3 (round 2):
        // one HBM pass instead of two
        // (2^11 and 2^12 only: 1.09 vs 1.46 and 1.33 vs 1.42 ms per 3 * 2^26 words; at 2^13 / 2^14 the limbs of a slice sit in
        // different workgroups and the 24-byte element stride costs more than the second pass saves: 1.52 vs 1.42, 1.78 vs 1.33)
        if (log_n <= (s.L == 1 ? 14 : 12) && (s.L == 1 || s.L == 3) && s.cosets == 1 && min_passes == 0 &&
            s.batch < (size_t(1) << 29)) {
            // the inverse transform of a BFieldElement product (second operand on load) is the one shape that truncates its store
            const bool product = product_inverse && s.L == 1;
            if (product || (!s.in2 && s.n_out < 0 && !(load_work && s.inverse) && !(s.post_scale && !s.inverse))) {
                p.truncates = product;
                return take(NttRoute::Block, 1);
            }
        }
    }
    // multi-pass: n = N_1 * ... * N_P, every N_i = 2^(a_i) <= 1024.  Passes 1 .. P-1 are column passes (DFT over digit i,
    // inter-pass twiddle, same position in and out); the last pass transforms the contiguous rows of N_P elements and
    // scatters output digit k_P to  k_1 + N_1 k_2 + ... + N_1..N_{P-1} k_P  (natural order).
    p.narrow = !large && small_launch_for(s);
    if (p.narrow) p.wg = 256;
    p.P = pass_count(log_n);
    choose_split(log_n, p.P, s.L, p.a);
    // 2^21 and 2^22 points in TWO passes: a 2048-point pass runs as pairs of 1024-point workgroups that share their input
    // (ntt_kernels.h, PRE2; a[i] = 11 below)
    if (pre2_plan_ok(s, log_n, p)) {
        p.P = 2;
        // (a scaling first pass on the one-workgroup kernel needs the offset itself, for the inter-pass table with offset^b folded in)
        p.c8 = c8_first_pass(log_n, s.pre_scale) && (!s.pre_scale || s.coset_offset);
        pre2_split(log_n, p.a, p.c8);
        p.pre2[0] = p.a[0] == 11 && !p.c8, p.pre2[1] = p.a[1] == 11;
    }
    const int P = p.P, last = p.a[P - 1];
    // batch tiles: as many polynomials as the scratch budget between the passes holds
    const size_t poly_bytes = s.n * s.cosets * size_t(s.L) * sizeof(u64);
    p.tb = std::min(std::max<size_t>(1, g_tile_bytes / poly_bytes), s.batch);
    p.ntiles = (s.batch + p.tb - 1) / p.tb;
    p.tb = (s.batch + p.ntiles - 1) / p.ntiles;  // equal tiles: 64 polynomials at 21 per tile are 4 x 16, not 21 + 21 + 21 + 1
    // pipelined tiles (g_pipe): tile t runs on side stream t % K with scratch tile t % K.
    // Automatic (round 6, profiles/r06_pipe_tiles.txt): two streams for the two-pass plans of 2^21 / 2^22 points -- their first pass is bound
    // by the memory pipe (0.68-0.76 of the issue slots busy) and their last pass by the vector ALU (0.80), so tile t + 1's first pass beside
    // tile t's last pass gains 2.6-3.4 % (configs[3] 7.27-7.36 -> 7.06-7.08 ms, 64 x 2^22 XFE ntt 6.67 -> 6.49) -- and one stream for
    // everything else (1024 x 2^20 BFE: 7.20-7.30 vs 7.24-7.32 ms, both passes VALU-bound).
    int pipe = g_pipe.load(std::memory_order_relaxed);
    if (pipe <= 0) pipe = (P == 2 && log_n >= 21) ? 2 : 1;
    p.K = (P < 4) ? (int)std::min<size_t>((size_t)pipe, p.ntiles) : 1;
    if (P < 4) {
        // (the narrow tiles take the generic last pass; the kernel's variant that multiplies on store serves fast_coset_interpolate)
        p.plain1024 = (last == 10 || p.pre2[P - 1]) && !p.narrow && (!s.post_scale || (s.inverse && log_n <= 28));
        // XFieldElement rows through the R = 1024 kernel: word-granular tiles (whole 128-byte lines on the output side)
        // (the other last-pass kernels too: all their thread slots as word-columns, e.g. 32 words = 256 bytes for R = 512)
        if (s.L == 3) {
            if (p.plain1024) {
                p.words = 16;
            } else {  // share the N_1 * L words of a row evenly among the fewest tiles, in whole lines
                const long long tot = (1ll << p.a[0]) * (long long)s.cosets * s.L, wmax = std::max(16, p.wg >> (last - 5));
                const long long tiles_per_row = (tot + wmax - 1) / wmax;
                p.words = (int)((((tot + tiles_per_row - 1) / tiles_per_row) + 15) / 16 * 16);
            }
        }
    }
    // the LAST1024 kernel (two or three passes, last radix 1024) is the one that truncates, and it addresses its stores through a
    // buffer resource: 1024 * (n L / 1024) * 8 bytes must fit 32 bits (fits_buffer_offsets)
    p.truncates = P <= 3 && last == 10 && !p.narrow && (unsigned long long)s.n * s.L * 8 + (1ull << 20) < (1ull << 32);
    // (the last pass of a four-pass plan is launched per polynomial)
    return take(NttRoute::Passes, P == 4 ? p.ntiles * 3 + s.batch : p.ntiles * P);
}

NttPlan plan_ntt(const NttShape& s) { return plan_call(s, false); }

NttPlan plan_ntt_large(size_t n, int L) {
    NttShape s;
    s.n = n, s.batch = 1, s.L = L;
    return plan_call(s, true);
}

// Can the inverse transform of an n-point product truncate its output (n_out >= 0 in run_ntt)?  The shape fast_multiply sends:
// over BFieldElement the pointwise product rides on the first load (in2).
bool can_truncate(size_t n, int L) {
    if (n <= 1024) return false;
    NttShape s;
    s.n = n, s.batch = 1, s.L = L, s.inverse = true, s.in2 = L == 1, s.n_out = (long long)n, s.packed = false;
    return plan_ntt(s).truncates;
}

// Blown-up evaluation (n_coeffs <= order / 2, the low-degree-extension shape): when the padded coefficient length
// needs one global pass fewer than the order (len <= 2^20 < order), evaluate on the order / len cosets of the
// subgroup of size len instead of transforming zeros.  Same values: exact arithmetic.  Measured (tools/lde_shapes.py):
// 2^18 -> 2^21 2.94 vs 3.47 ms, 2^20 -> 2^23 2.80 vs 3.71 ms per 2^28 points; with equal pass counts the plain plan
// wins because its first pass skips the zero rows, so it stays the default there.
size_t coset_split(size_t n_coeffs, size_t order, size_t batch, int L) {
    size_t len = 1;
    while (len < n_coeffs) len <<= 1;
    // ADVICE r3 asked whether the comparison should use the EFFECTIVE pass count of the plain plan (orders 2^21 / 2^22 run in two
    // passes under PRE2, so the split then saves no pass).  Built and measured (profiles/r04_lde_split_rule.txt, 2^28 words per
    // call): the split still wins where it matters -- BFE 2^20 -> 2^22 2.05 vs 2.48 ms, 2^19 -> 2^22 2.03 vs 2.40, 2^20 -> 2^21
    // 2.07 vs 2.17; XFE 2^20 -> 2^22 1.01 vs 1.13 -- because its first pass reads n_coeffs rows instead of `order` and none of its
    // passes pays the PRE2 pair's second read and second scaling; only XFE 2^18 / 2^19 -> 2^21 is 3 % faster on the plain plan.
    // The round-3 rule (nominal pass counts) therefore stays.
    const int plain_passes = pass_count(ilog2(order));
    // (at most kMaxCosetSplit cosets: one scale table of n_coeffs words per coset is built and, while it fits the budget, cached)
    const bool split = len > 1024 && len < order && order / len <= kMaxCosetSplit && order <= (size_t(1) << 30) &&
                       pass_count(ilog2(len)) < plain_passes;
    return split ? order / len : 1;
}

}  // namespace tfi
