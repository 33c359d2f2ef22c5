/* Host side of K35's entry points (dmh_sgm_plan, dmh_sgm_disparity) under AddressSanitizer, as tests/asan/hint_checks.c does it for
 * K34: linked against libdmh_hip_asan.so (host code only, no device code).  Every argument check: each call below must be refused on
 * the host before any launch, and the plan's sizes are checked against the layout the header states.  Compiled as C.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "dmh_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "sgm_checks: %s (line %d): %s\n", #cond, __LINE__, dmh_last_error()); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

static int64_t up(int64_t v) { return (v + 255) / 256 * 256; }

int main(void) {
    void* one = (void*)(uintptr_t)256;      /* non-NULL, 256-byte aligned dummy "device pointers" */
    void* two = (void*)(uintptr_t)512;
    void* by2 = (void*)(uintptr_t)258;      /* 2-byte aligned only */
    void* odd = (void*)(uintptr_t)257;
    void* by64 = (void*)(uintptr_t)320;     /* not 256-byte aligned */
    const uint8_t* img = (const uint8_t*)odd;       /* bytes need no alignment */
    const uint8_t* img2 = (const uint8_t*)(uintptr_t)4097;
    const int32_t* rev = (const int32_t*)(uintptr_t)1024;
    const int nums[4] = {64, 96, 128, 160};
    dmh_sgm_params twelve[12], p[17];
    int chunks = -1, i;
    int64_t per_item = 0;

    EXPECT(DMH_SGM_MAX_MATCHERS == 16 && DMH_SGM_MAX_WIDTH == 4096);
    for (i = 0; i < 12; ++i) {              /* the reference's parameter sets */
        dmh_sgm_params q = {0, 0, 36, 288, 63, 10, 0, 100, 16, 0};
        q.num_disparities = nums[i % 4];
        q.block_size = 1 + i / 4;
        twelve[i] = q;
    }
    for (i = 0; i < 17; ++i) p[i] = twelve[i % 12];

    /* the plan: 8 distinct sets per item (blockSize 2 and 3 share a radius) */
    for (i = 0; i < 4; ++i) per_item += 2 * (2 * up(2ll * 16 * (208 - nums[i]) * nums[i]) + up(8ll * 16 * 208));
    EXPECT(dmh_sgm_plan(3, 16, 208, twelve, 12, (int64_t)2 << 30, &chunks) == 3 * per_item && chunks == 1);
    EXPECT(dmh_sgm_plan(5, 16, 208, twelve, 12, (int64_t)2 << 30, &chunks) == 4 * per_item && chunks == 2);      /* 40 jobs: 32 + 8 */
    EXPECT(dmh_sgm_plan(3, 16, 208, twelve, 12, (int64_t)3 << 20, &chunks) <= ((int64_t)3 << 20) && chunks == 6);
    EXPECT(dmh_sgm_plan(3, 16, 208, twelve, 12, (int64_t)2 << 30, NULL) == 3 * per_item);
    EXPECT(dmh_sgm_plan(8, 320, 1024, twelve, 12, (int64_t)2 << 30, &chunks) <= ((int64_t)2 << 30) && chunks == 4);
    EXPECT(dmh_sgm_plan(3, 16, 208, twelve, 12, 1 << 16, &chunks) == -1);
    EXPECT(strstr(dmh_last_error(), "cap") != NULL);
    EXPECT(dmh_sgm_plan(3, 16, 208, twelve, 12, 0, &chunks) == -1);
    EXPECT(dmh_sgm_plan(1, 16, 64, twelve, 1, 1 << 20, &chunks) == up(8ll * 16 * 64) && chunks == 1);           /* W <= D: labels only */
    EXPECT(dmh_sgm_plan(0, 16, 208, twelve, 12, (int64_t)2 << 30, &chunks) == -1);
    EXPECT(dmh_sgm_plan(3, 16, 4097, twelve, 12, (int64_t)2 << 30, &chunks) == -1);
    EXPECT(strstr(dmh_last_error(), "4096") != NULL);
    EXPECT(dmh_sgm_plan(3, 65536, 20, twelve, 12, (int64_t)2 << 30, &chunks) == -1);
    EXPECT(dmh_sgm_plan(3, 16, 208, NULL, 12, (int64_t)2 << 30, &chunks) == -1);
    EXPECT(dmh_sgm_plan(3, 16, 208, p, 17, (int64_t)2 << 30, &chunks) == -1);
    EXPECT(strstr(dmh_last_error(), "N <= 16") != NULL);
    EXPECT(dmh_sgm_plan(3, 16, 208, twelve, 0, (int64_t)2 << 30, &chunks) == -1);
    EXPECT(dmh_sgm_plan(64, 2048, 4096, twelve, 12, (int64_t)1 << 40, &chunks) == -1);                           /* B N H W >= 2^31 */
    EXPECT(strstr(dmh_last_error(), "2^31") != NULL);

    /* a good call's arguments, each broken in turn (3 pairs of 16 x 208, twelve sets) */
#define RUN(base, lookup, reverse, B, H, W, params, N, out, ws, bytes) \
    dmh_sgm_disparity(base, lookup, reverse, B, H, W, params, N, (int16_t*)(out), ws, bytes, DMH_SGM_ALL, NULL)
    EXPECT(RUN(NULL, img2, rev, 3, 16, 208, twelve, 12, two, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "null pointer") != NULL);
    EXPECT(RUN(img, NULL, rev, 3, 16, 208, twelve, 12, two, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 3, 16, 208, twelve, 12, NULL, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 3, 16, 208, twelve, 12, two, NULL, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 3, 16, 208, NULL, 12, two, one, 3 * per_item) == DMH_EINVAL);
    /* N, shapes */
    EXPECT(RUN(img, img2, rev, 3, 16, 208, p, 17, two, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 3, 16, 208, twelve, 0, two, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 3, 16, 208, twelve, -2, two, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 0, 16, 208, twelve, 12, two, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 3, 0, 208, twelve, 12, two, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 3, 16, -208, twelve, 12, two, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 3, 16, 4097, twelve, 12, two, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 3, 65536, 208, twelve, 12, two, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 64, 2048, 4096, twelve, 12, two, one, 3 * per_item) == DMH_EINVAL);
    /* alignment, aliases, the workspace */
    EXPECT(RUN(img, img2, rev, 3, 16, 208, twelve, 12, odd, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "aligned") != NULL);
    EXPECT(RUN(img, img2, (const int32_t*)by2, 3, 16, 208, twelve, 12, two, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 3, 16, 208, twelve, 12, two, by64, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 3, 16, 208, twelve, 12, one, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "alias") != NULL);
    EXPECT(RUN((const uint8_t*)two, img2, rev, 3, 16, 208, twelve, 12, two, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, (const uint8_t*)one, rev, 3, 16, 208, twelve, 12, two, one, 3 * per_item) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 3, 16, 208, twelve, 12, two, one, 0) == DMH_EINVAL);
    EXPECT(RUN(img, img2, rev, 3, 16, 208, twelve, 12, two, one, 1 << 16) == DMH_EINVAL);           /* less than one job needs */
    EXPECT(strstr(dmh_last_error(), "workspace") != NULL);

    EXPECT(dmh_sgm_disparity(img, img2, rev, 3, 16, 208, twelve, 12, (int16_t*)two, one, 3 * per_item, 0, NULL) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "phases") != NULL);
    EXPECT(dmh_sgm_disparity(img, img2, rev, 3, 16, 208, twelve, 12, (int16_t*)two, one, 3 * per_item, 16, NULL) == DMH_EINVAL);
    EXPECT(DMH_SGM_ALL == (DMH_SGM_COST | DMH_SGM_PATHS | DMH_SGM_SELECT | DMH_SGM_SPECKLE));

    /* every parameter refusal, through both entry points */
#define BAD(field, value, text)                                                                         \
    do {                                                                                                \
        dmh_sgm_params q[2];                                                                            \
        q[0] = twelve[0];                                                                               \
        q[1] = twelve[11];                                                                              \
        q[1].field = (value);                                                                           \
        EXPECT(dmh_sgm_plan(3, 16, 208, q, 2, (int64_t)2 << 30, NULL) == -1);                           \
        EXPECT(strstr(dmh_last_error(), text) != NULL);                                                 \
        EXPECT(RUN(img, img2, rev, 3, 16, 208, q, 2, two, one, 3 * per_item) == DMH_EINVAL);            \
        EXPECT(strstr(dmh_last_error(), text) != NULL);                                                 \
    } while (0)
    BAD(block_size, 5, "blockSize");
    BAD(block_size, 4, "blockSize");
    BAD(block_size, 0, "blockSize");
    BAD(num_disparities, 24, "multiple of 16");
    BAD(num_disparities, 0, "multiple of 16");
    BAD(num_disparities, 272, "multiple of 16");
    BAD(num_disparities, -16, "multiple of 16");
    BAD(min_disparity, 1, "minDisparity");
    BAD(min_disparity, -16, "minDisparity");
    BAD(P1, -1, "P1");
    BAD(P2, -1, "P2");
    BAD(P2, 1451, "32767");                 /* 5 (9 x 567 + 1451) = 32770 */
    BAD(P2, 2147483647, "32767");
    BAD(pre_filter_cap, 0, "preFilterCap");
    BAD(pre_filter_cap, 64, "preFilterCap");
    BAD(uniqueness_ratio, -1, "uniquenessRatio");
    BAD(uniqueness_ratio, 101, "uniquenessRatio");
    BAD(disp12_max_diff, -1, "disp12MaxDiff");
    BAD(speckle_window_size, -1, "speckleWindowSize");
    BAD(speckle_range, -1, "speckleRange");
    BAD(speckle_range, 4097, "speckleRange");
    {
        dmh_sgm_params q = twelve[11];
        q.P2 = 1450;                        /* 5 (9 x 567 + 1450) = 32765: the last P2 served at radius 1 */
        EXPECT(dmh_sgm_plan(1, 16, 208, &q, 1, (int64_t)2 << 30, &chunks) > 0 && chunks == 1);
        q.block_size = 1;
        q.P2 = 5986;                        /* 5 (567 + 5986) = 32765 at radius 0 */
        EXPECT(dmh_sgm_plan(1, 16, 208, &q, 1, (int64_t)2 << 30, &chunks) > 0);
        q.P2 = 5987;
        EXPECT(dmh_sgm_plan(1, 16, 208, &q, 1, (int64_t)2 << 30, &chunks) == -1);
    }
    if (failures) {
        fprintf(stderr, "sgm_checks: %d failure(s)\n", failures);
        return 1;
    }
    printf("sgm_checks: ok\n");
    return 0;
}
