// The host-side plan the reduction files share (simpleinfer_amd/csrc/hip/si_reduce_plan.h): the fold of {n, h, w} under a mask into kept and
// reduced levels against a brute-force count, the lanes-per-row rule against its written-out loop, the output pixel count, each side of each
// limit of the shared descriptor check, and the kernel-name helper against the 56 strings the three name tables used to spell by hand.
// Stand-alone; built with -fsanitize=address,undefined by tests/test_reduce_plan_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "si_reduce_plan.h"

static long long failures = 0, checked = 0;

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        ++checked;                                                                    \
        if (!(cond) && ++failures <= 20) std::printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

// All seven non-empty spatial masks x n, h, w in {1, 2, 3, 5}.  Kept index kp and position r each count their axes in increasing (n, h, w)
// order, the last axis fastest: the pixel the levels give must be the pixel of that NHWC index, and the pairs must hit every pixel once.
static void test_fold_against_brute_force() {
    const int sizes[] = {1, 2, 3, 5};
    long long cases = 0;
    for (int axes = 1; axes <= 7; ++axes)
        for (int n : sizes)
            for (int h : sizes)
                for (int w : sizes) {
                    ++cases;
                    const int ext[3] = {n, h, w};
                    const SiLevels lv = si_fold_levels(n, h, w, axes);
                    const SiLevelArgs a = si_level_args(lv);
                    long long kept = 1, red = 1;
                    for (int x = 0; x < 3; ++x) (((axes >> x) & 1) ? red : kept) *= ext[x];
                    EXPECT((long long)lv.kept[0][0] * lv.kept[1][0] == kept);
                    EXPECT((long long)lv.positions == red && a.R == red);
                    EXPECT((long long)lv.red[0][0] * lv.red[1][0] == red);
                    EXPECT(a.K1 == lv.kept[1][0] && a.ks0 == lv.kept[0][1] && a.ks1 == lv.kept[1][1]);
                    EXPECT(a.R1 == lv.red[1][0] && a.rs0 == lv.red[0][1] && a.rs1 == lv.red[1][1]);
                    EXPECT(si_masked_pixels(n, h, w, axes) == (uint64_t)kept);
                    std::vector<int> hits((size_t)n * h * w, 0);
                    for (long long kp = 0; kp < kept; ++kp)
                        for (long long r = 0; r < red; ++r) {
                            // the NHWC index: digits of kp over the kept axes and of r over the reduced ones, last axis fastest
                            int idx[3];
                            long long k = kp, q = r;
                            for (int x = 2; x >= 0; --x) {
                                long long& from = ((axes >> x) & 1) ? q : k;
                                idx[x] = (int)(from % ext[x]);
                                from /= ext[x];
                            }
                            const long long want = ((long long)idx[0] * h + idx[1]) * w + idx[2];
                            const long long got = (kp / a.K1) * a.ks0 + (kp % a.K1) * a.ks1 + (r / a.R1) * a.rs0 + (r % a.R1) * a.rs1;
                            EXPECT(got == want);
                            if (got >= 0 && got < (long long)hits.size()) ++hits[(size_t)got];
                        }
                    bool once = true;
                    for (int c : hits) once = once && c == 1;
                    EXPECT(once);
                }
    EXPECT(cases == 448);
    // no axis: one position, every pixel kept as one run
    const SiLevelArgs none = si_level_args(si_fold_levels(2, 3, 5, 0));
    EXPECT(none.R == 1 && none.R1 == 1 && none.K1 == 30 && none.ks1 == 1);
    const SiLevelArgs dflt;
    EXPECT(dflt.K1 == 1 && dflt.ks0 == 0 && dflt.ks1 == 0 && dflt.R == 1 && dflt.R1 == 1 && dflt.rs0 == 0 && dflt.rs1 == 0);
    std::printf("%lld fold cases\n", cases);
}

static void test_masked_pixels() {
    EXPECT(si_masked_pixels(2, 3, 5, 0) == 30);
    EXPECT(si_masked_pixels(2, 3, 5, SI_AXIS_N) == 15 && si_masked_pixels(2, 3, 5, SI_AXIS_H) == 10 && si_masked_pixels(2, 3, 5, SI_AXIS_W) == 6);
    EXPECT(si_masked_pixels(2, 3, 5, SI_AXIS_H | SI_AXIS_W) == 2 && si_masked_pixels(2, 3, 5, SI_AXIS_SPATIAL) == 1);
    EXPECT(si_masked_pixels(2, 3, 5, SI_AXIS_C) == 30 && si_masked_pixels(2, 3, 5, SI_AXIS_C | SI_AXIS_N) == 15);   // c is no pixel axis
    EXPECT(si_masked_pixels(65536, 65536, 4, 0) == (1ull << 34));                                                    // 64-bit product
    EXPECT(SI_AXIS_N == 1 && SI_AXIS_H == 2 && SI_AXIS_W == 4 && SI_AXIS_C == 8 && SI_AXIS_SPATIAL == 7);
}

static void test_group_lg() {
    for (int per : {1, 2, 4})
        for (int cv = 1; cv <= 300; ++cv) {
            int lg = 0;
            while ((1 << lg) < 64 && (1 << lg) * per < cv) ++lg;
            EXPECT(si_group_lg(cv, per) == lg);
        }
    EXPECT(si_group_lg(1, 4) == 0 && si_group_lg(5, 4) == 1 && si_group_lg(256, 4) == 6 && si_group_lg(100000, 4) == 6);
}

static void test_shared_check() {
    const int L = (int)SI_INDEX_LIMIT;
    const int OK = 0, BAD = SI_PLAN_BADARG, UNS = SI_PLAN_UNSUPPORTED;
    EXPECT(BAD == -1 && UNS == -2);
    EXPECT(si_check_reduce_views(2, 3, 5, 8, 8, 8, 30, 8) == OK);
    // extents
    EXPECT(si_check_reduce_views(0, 3, 5, 8, 8, 8, 30, 8) == BAD && si_check_reduce_views(2, 0, 5, 8, 8, 8, 30, 8) == BAD);
    EXPECT(si_check_reduce_views(2, 3, 0, 8, 8, 8, 30, 8) == BAD && si_check_reduce_views(2, 3, 5, 0, 8, 8, 30, 8) == BAD);
    EXPECT(si_check_reduce_views(-1, 3, 5, 8, 8, 8, 30, 8) == BAD);
    // strides against channel counts
    EXPECT(si_check_reduce_views(2, 3, 5, 8, 7, 8, 30, 8) == BAD && si_check_reduce_views(2, 3, 5, 8, 8, 7, 30, 8) == BAD);
    EXPECT(si_check_reduce_views(2, 3, 5, 8, 8, 1, 30, 1) == OK && si_check_reduce_views(2, 3, 5, 8, 8, 0, 30, 1) == BAD);
    // a bad argument is found before a tensor that is too wide
    EXPECT(si_check_reduce_views(L, 2, 1, 1, 0, 1, 1, 1) == BAD);
    // rows = n * h at the limit and one above (w = 1, ld = 1: nothing else is beyond it)
    EXPECT(si_check_reduce_views(L, 1, 1, 1, 1, 1, 1, 1) == OK);
    EXPECT(si_check_reduce_views(1 << 16, 1 << 15, 1, 1, 1, 1, 1, 1) == UNS);   // rows = 2^31 = L + 1
    EXPECT(si_check_reduce_views(L, L, 1, 1, 1, 1, 1, 1) == UNS);               // rows < 2^62: no wrap on the way
    // pix = rows * w
    EXPECT(si_check_reduce_views(1, 1, L, 1, 1, 1, 1, 1) == OK);
    EXPECT(si_check_reduce_views(1, 1 << 15, 1 << 16, 1, 1, 1, 1, 1) == UNS);   // rows = 2^15 fits, pix = 2^31 = L + 1
    // pix * in_ld: L = 2147483647 = 7 * 306783378 + 1
    EXPECT(si_check_reduce_views(1, 1, 306783378, 7, 7, 1, 1, 1) == OK);        // 7 * 306783378 = L - 1
    EXPECT(si_check_reduce_views(1, 1, 1, 1, L, 1, 1, 1) == OK);                // pix * in_ld = L (a prime: one pixel, or ld = 1 above)
    EXPECT(si_check_reduce_views(1, 1, (L - 1) / 2 + 1, 1, 2, 1, 1, 1) == UNS); // 2 * 2^30 = L + 1
    EXPECT(si_check_reduce_views(1, 1, (L - 1) / 2, 1, 2, 1, 1, 1) == OK);      // 2 * (2^30 - 1) = L - 1
    // opix * out_ld
    EXPECT(si_check_reduce_views(1, 1, 1, 1, 1, 1, (uint64_t)L, 1) == OK);
    EXPECT(si_check_reduce_views(1, 1, 1, 1, 1, 1, (uint64_t)L + 1, 1) == UNS);
    EXPECT(si_check_reduce_views(1, 1, 1, 1, 1, L, 1, 1) == OK);
    EXPECT(si_check_reduce_views(1, 1, 1, 1, 1, 2, 1ull << 30, 1) == UNS);      // 2 * 2^30 = L + 1
}

static void test_kernel_names() {
    // the three tables as the files spelled them before the helper
    static const char* const parent[14][4] = {
        {"softmax_group_kernel<float, 4>", "softmax_group_kernel<float, 1>", "softmax_group_kernel<_Float16, 8>", "softmax_group_kernel<_Float16, 1>"},
        {"softmax_block_kernel<float, 4>", "softmax_block_kernel<float, 1>", "softmax_block_kernel<_Float16, 8>", "softmax_block_kernel<_Float16, 1>"},
        {"softmax_block_online_kernel<float, 4>", "softmax_block_online_kernel<float, 1>", "softmax_block_online_kernel<_Float16, 8>",
         "softmax_block_online_kernel<_Float16, 1>"},
        {"softmax_strided_kernel<float, 4>", "softmax_strided_kernel<float, 1>", "softmax_strided_kernel<_Float16, 8>",
         "softmax_strided_kernel<_Float16, 1>"},
        {"softmax_strided_online_kernel<float, 4>", "softmax_strided_online_kernel<float, 1>", "softmax_strided_online_kernel<_Float16, 8>",
         "softmax_strided_online_kernel<_Float16, 1>"},
        {"reduce_row_group_kernel<float, 4>", "reduce_row_group_kernel<float, 1>", "reduce_row_group_kernel<_Float16, 8>",
         "reduce_row_group_kernel<_Float16, 1>"},
        {"reduce_row_block_kernel<float, 4>", "reduce_row_block_kernel<float, 1>", "reduce_row_block_kernel<_Float16, 8>",
         "reduce_row_block_kernel<_Float16, 1>"},
        {"reduce_col_lane_kernel<float, 4>", "reduce_col_lane_kernel<float, 1>", "reduce_col_lane_kernel<_Float16, 8>",
         "reduce_col_lane_kernel<_Float16, 1>"},
        {"reduce_col_coop_kernel<float, 4>", "reduce_col_coop_kernel<float, 1>", "reduce_col_coop_kernel<_Float16, 8>",
         "reduce_col_coop_kernel<_Float16, 1>"},
        {"lpnorm_row_group_kernel<float, 4>", "lpnorm_row_group_kernel<float, 1>", "lpnorm_row_group_kernel<_Float16, 8>",
         "lpnorm_row_group_kernel<_Float16, 1>"},
        {"lpnorm_row_block_kernel<float, 4>", "lpnorm_row_block_kernel<float, 1>", "lpnorm_row_block_kernel<_Float16, 8>",
         "lpnorm_row_block_kernel<_Float16, 1>"},
        {"lpnorm_row_block_2pass_kernel<float, 4>", "lpnorm_row_block_2pass_kernel<float, 1>", "lpnorm_row_block_2pass_kernel<_Float16, 8>",
         "lpnorm_row_block_2pass_kernel<_Float16, 1>"},
        {"lpnorm_col_lane_kernel<float, 4>", "lpnorm_col_lane_kernel<float, 1>", "lpnorm_col_lane_kernel<_Float16, 8>",
         "lpnorm_col_lane_kernel<_Float16, 1>"},
        {"lpnorm_col_lane_reg_kernel<float, 4>", "lpnorm_col_lane_reg_kernel<float, 1>", "lpnorm_col_lane_reg_kernel<_Float16, 8>",
         "lpnorm_col_lane_reg_kernel<_Float16, 1>"},
    };
    static const char* const helper[14][4] = {
        SI_KERNEL_NAMES("softmax_group_kernel"), SI_KERNEL_NAMES("softmax_block_kernel"), SI_KERNEL_NAMES("softmax_block_online_kernel"),
        SI_KERNEL_NAMES("softmax_strided_kernel"), SI_KERNEL_NAMES("softmax_strided_online_kernel"),
        SI_KERNEL_NAMES("reduce_row_group_kernel"), SI_KERNEL_NAMES("reduce_row_block_kernel"), SI_KERNEL_NAMES("reduce_col_lane_kernel"),
        SI_KERNEL_NAMES("reduce_col_coop_kernel"),
        SI_KERNEL_NAMES("lpnorm_row_group_kernel"), SI_KERNEL_NAMES("lpnorm_row_block_kernel"), SI_KERNEL_NAMES("lpnorm_row_block_2pass_kernel"),
        SI_KERNEL_NAMES("lpnorm_col_lane_kernel"), SI_KERNEL_NAMES("lpnorm_col_lane_reg_kernel"),
    };
    int same = 0;
    for (int f = 0; f < 14; ++f)
        for (int k = 0; k < 4; ++k) same += 0 == std::strcmp(parent[f][k], helper[f][k]);
    EXPECT(same == 56);
    // the entry a launch picks, as the tables were indexed: (half ? 2 : 0) + (vec ? 0 : 1)
    EXPECT(si_kernel_name_index(false, true) == 0 && si_kernel_name_index(false, false) == 1);
    EXPECT(si_kernel_name_index(true, true) == 2 && si_kernel_name_index(true, false) == 3);
}

int main() {
    test_fold_against_brute_force();
    test_masked_pixels();
    test_group_lg();
    test_shared_check();
    test_kernel_names();
    if (failures) {
        std::printf("%lld of %lld checks failed\n", failures, checked);
        return 1;
    }
    std::printf("reduce plan ok (%lld checks)\n", checked);
    return 0;
}
