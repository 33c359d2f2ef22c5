/* Host side of K32's entry points (dmh_velo_depth_ws_size, dmh_velo_depth_map) under AddressSanitizer, as tests/asan/pil_checks.c
 * does it for K31: linked against libdmh_hip_asan.so (host code only, no device code).  Workspace sizes and every argument check:
 * each launch call below must be refused on the host before any launch.  Compiled as C.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "dmh_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "velo_checks: %s (line %d): %s\n", #cond, __LINE__, dmh_last_error()); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

int main(void) {
    void* one = (void*)(uintptr_t)64;       /* a non-NULL, 16-byte aligned dummy "device pointer" */
    void* two = (void*)(uintptr_t)128;
    void* by4 = (void*)(uintptr_t)68;       /* 4-byte aligned only */
    void* odd = (void*)(uintptr_t)66;
    const int32_t* t = (const int32_t*)one;

    /* workspace: one word per cell, four per row (first and last index of columns 0 and W - 1) */
    EXPECT(dmh_velo_depth_ws_size(375 * 1242, 375) == 375 * 1242 + 4 * 375);
    EXPECT(dmh_velo_depth_ws_size(32ll * 375 * 1242, 32 * 375) == 32ll * 375 * 1242 + 4 * 32 * 375);
    EXPECT(dmh_velo_depth_ws_size(0, 1) == -1 && dmh_velo_depth_ws_size(1, 0) == -1 && dmh_velo_depth_ws_size(-5, 3) == -1);
    EXPECT(dmh_velo_depth_ws_size((int64_t)1 << 31, 1) == -1);
    EXPECT(dmh_velo_depth_ws_size(((int64_t)1 << 31) - 4, 1) == -1 && dmh_velo_depth_ws_size(((int64_t)1 << 31) - 5, 1) == ((int64_t)1 << 31) - 1);

    /* a good call's arguments, each broken in turn (two frames of 38 x 124, 6000 points, to 375 x 1242) */
#define CALL(pts, npts, off, proj, desc, flip, n, cells, rows, oh, ow, ws, out) \
    dmh_velo_depth_map((const float*)(pts), npts, off, (const double*)(proj), desc, flip, n, 0, cells, rows, oh, ow, (uint32_t*)(ws), (float*)(out), NULL)
    EXPECT(CALL(one, 6000, NULL, one, t, NULL, 2, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "null pointer") != NULL);
    EXPECT(CALL(one, 6000, t, NULL, t, NULL, 2, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);
    EXPECT(CALL(one, 6000, t, one, NULL, NULL, 2, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, 2, 9424, 76, 375, 1242, NULL, two) == DMH_EINVAL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, 2, 9424, 76, 375, 1242, one, NULL) == DMH_EINVAL);
    EXPECT(CALL(NULL, 6000, t, one, t, NULL, 2, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);      /* points may be NULL only with npts == 0 */
    EXPECT(strstr(dmh_last_error(), "null points") != NULL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, 0, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, (1 << 20) + 1, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);
    EXPECT(CALL(one, -1, t, one, t, NULL, 2, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);
    EXPECT(CALL(one, (int64_t)1 << 31, t, one, t, NULL, 2, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "2^31") != NULL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, 2, 0, 76, 375, 1242, one, two) == DMH_EINVAL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, 2, 9424, 0, 375, 1242, one, two) == DMH_EINVAL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, 2, (int64_t)1 << 31, 76, 375, 1242, one, two) == DMH_EINVAL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, 2, 9424, 76, 375, 0, one, two) == DMH_EINVAL);          /* one of out_h, out_w only */
    EXPECT(strstr(dmh_last_error(), "both") != NULL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, 2, 9424, 76, -1, -1, one, two) == DMH_EINVAL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, 5000, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);    /* 5000 x 375 x 1242 >= 2^31 */
    EXPECT(strstr(dmh_last_error(), "output") != NULL);
    EXPECT(CALL(by4, 6000, t, one, t, NULL, 2, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);       /* points are read as 16-byte vectors */
    EXPECT(strstr(dmh_last_error(), "16-byte") != NULL);
    EXPECT(CALL(one, 6000, t, by4, t, NULL, 2, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);       /* proj is float64 */
    EXPECT(CALL(one, 6000, (const int32_t*)odd, one, t, NULL, 2, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);
    EXPECT(CALL(one, 6000, t, one, (const int32_t*)odd, NULL, 2, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);
    EXPECT(CALL(one, 6000, t, one, t, (const int32_t*)odd, 2, 9424, 76, 375, 1242, one, two) == DMH_EINVAL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, 2, 9424, 76, 375, 1242, odd, two) == DMH_EINVAL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, 2, 9424, 76, 375, 1242, one, odd) == DMH_EINVAL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, 2, 9424, 76, 375, 1242, two, two) == DMH_EINVAL);       /* out aliases ws */
    EXPECT(strstr(dmh_last_error(), "alias") != NULL);
    EXPECT(CALL(one, 6000, t, one, t, NULL, 2, 9424, 76, 0, 0, two, one) == DMH_EINVAL);            /* out aliases points */
    if (failures) {
        fprintf(stderr, "velo_checks: %d failure(s)\n", failures);
        return 1;
    }
    printf("velo_checks: ok\n");
    return 0;
}
