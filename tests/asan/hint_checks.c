/* Host side of K34's entry points (dmh_depth_hint_fuse, dmh_depth_hint_prepare) under AddressSanitizer, as tests/asan/velo_checks.c
 * does it for K32: linked against libdmh_hip_asan.so (host code only, no device code).  Every argument check: each call below must
 * be refused on the host before any launch.  Compiled as C.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "dmh_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "hint_checks: %s (line %d): %s\n", #cond, __LINE__, dmh_last_error()); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

int main(void) {
    void* one = (void*)(uintptr_t)64;       /* non-NULL, aligned dummy "device pointers" */
    void* two = (void*)(uintptr_t)128;
    void* three = (void*)(uintptr_t)192;
    void* by2 = (void*)(uintptr_t)66;       /* 2-byte aligned only */
    void* odd = (void*)(uintptr_t)65;
    const uint8_t* img = (const uint8_t*)odd;      /* bytes need no alignment */
    const float* m = (const float*)one;
    const int32_t* t = (const int32_t*)one;

    EXPECT(DMH_HINT_MAX_CANDIDATES == 16);
    /* a good call's arguments, each broken in turn (8 pairs of 320 x 1024, 12 candidates) */
#define FUSE(base, lookup, cand, raw, K, iK, T, B, N, H, W, best, losses) \
    dmh_depth_hint_fuse(base, lookup, cand, raw, K, iK, T, B, N, H, W, (float*)(best), (float*)(losses), NULL)
    EXPECT(FUSE(NULL, img, one, 1, m, m, m, 8, 12, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "null pointer") != NULL);
    EXPECT(FUSE(img, NULL, one, 1, m, m, m, 8, 12, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, NULL, 1, m, m, m, 8, 12, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 1, NULL, m, m, 8, 12, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 1, m, NULL, m, 8, 12, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 1, m, m, NULL, 8, 12, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 1, m, m, m, 8, 12, 320, 1024, NULL, NULL) == DMH_EINVAL);
    /* N out of range */
    EXPECT(FUSE(img, img, one, 1, m, m, m, 8, 0, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "candidates") != NULL);
    EXPECT(FUSE(img, img, one, 1, m, m, m, 8, 17, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 1, m, m, m, 8, -3, 320, 1024, two, NULL) == DMH_EINVAL);
    /* shapes */
    EXPECT(FUSE(img, img, one, 1, m, m, m, 0, 12, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 1, m, m, m, 65536, 12, 2, 2, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 1, m, m, m, 8, 12, 1, 1024, two, NULL) == DMH_EINVAL);            /* reflection needs two rows */
    EXPECT(strstr(dmh_last_error(), "H, W >= 2") != NULL);
    EXPECT(FUSE(img, img, one, 1, m, m, m, 8, 12, 320, 1, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 1, m, m, m, 8, 12, 320, -1024, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 1, m, m, m, 64, 16, 2048, 1024, two, NULL) == DMH_EINVAL);        /* 2^31 candidate elements */
    EXPECT(strstr(dmh_last_error(), "2^31") != NULL);
    EXPECT(FUSE(img, img, one, 1, m, m, m, 1, 1, 600000, 2, two, NULL) == DMH_EINVAL);           /* more than 65535 tile rows */
    /* the candidate form and its alignment */
    EXPECT(FUSE(img, img, one, 2, m, m, m, 8, 12, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "cand_is_raw") != NULL);
    EXPECT(FUSE(img, img, odd, 1, m, m, m, 8, 12, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, by2, 0, m, m, m, 8, 12, 320, 1024, two, NULL) == DMH_EINVAL);          /* float depths at a 2-byte address */
    EXPECT(strstr(dmh_last_error(), "aligned") != NULL);
    EXPECT(FUSE(img, img, one, 1, (const float*)by2, m, m, 8, 12, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 1, m, (const float*)by2, m, 8, 12, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 1, m, m, (const float*)by2, 8, 12, 320, 1024, two, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 1, m, m, m, 8, 12, 320, 1024, by2, NULL) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 1, m, m, m, 8, 12, 320, 1024, two, by2) == DMH_EINVAL);
    /* aliases */
    EXPECT(FUSE(img, img, one, 0, m, m, m, 8, 12, 320, 1024, one, NULL) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "alias") != NULL);
    EXPECT(FUSE(img, img, one, 0, m, m, m, 8, 12, 320, 1024, two, one) == DMH_EINVAL);
    EXPECT(FUSE(img, img, one, 0, m, m, m, 8, 12, 320, 1024, two, two) == DMH_EINVAL);

    /* dmh_depth_hint_prepare: 4 hints of 320 x 1024 to 192 x 640 */
#define PREP(src, flip, yt, xt, yl, xl, B, Hs, Ws, H, W, hint, mask) \
    dmh_depth_hint_prepare((const float*)(src), flip, yt, xt, yl, xl, B, Hs, Ws, H, W, (float*)(hint), (float*)(mask), NULL)
    EXPECT(PREP(NULL, NULL, t, t, 192, 640, 4, 320, 1024, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "null pointer") != NULL);
    EXPECT(PREP(one, NULL, NULL, t, 192, 640, 4, 320, 1024, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, NULL, 192, 640, 4, 320, 1024, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, t, 192, 640, 4, 320, 1024, 192, 640, NULL, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, t, 192, 640, 4, 320, 1024, 192, 640, two, NULL) == DMH_EINVAL);
    /* table sizes: they must be the output's H and W, not the source's and not swapped */
    EXPECT(PREP(one, NULL, t, t, 320, 1024, 4, 320, 1024, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "tables") != NULL);
    EXPECT(PREP(one, NULL, t, t, 640, 192, 4, 320, 1024, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, t, 191, 640, 4, 320, 1024, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, t, 192, 641, 4, 320, 1024, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, t, 0, 0, 4, 320, 1024, 192, 640, two, three) == DMH_EINVAL);
    /* shapes */
    EXPECT(PREP(one, NULL, t, t, 192, 640, 0, 320, 1024, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, t, 192, 640, 4, 0, 1024, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, t, 192, 640, 4, 320, -1, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, t, 0, 640, 4, 320, 1024, 0, 640, two, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, t, 40000, 40000, 4, 320, 1024, 40000, 40000, two, three) == DMH_EINVAL);   /* 4 x 1.6e9 outputs */
    EXPECT(strstr(dmh_last_error(), "2^31") != NULL);
    EXPECT(PREP(one, NULL, t, t, 2, 2, 4, 40000, 40000, 2, 2, two, three) == DMH_EINVAL);
    /* alignment and aliases */
    EXPECT(PREP(by2, NULL, t, t, 192, 640, 4, 320, 1024, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(PREP(one, (const int32_t*)by2, t, t, 192, 640, 4, 320, 1024, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, (const int32_t*)by2, t, 192, 640, 4, 320, 1024, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, (const int32_t*)by2, 192, 640, 4, 320, 1024, 192, 640, two, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, t, 192, 640, 4, 320, 1024, 192, 640, by2, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, t, 192, 640, 4, 320, 1024, 192, 640, two, by2) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, t, 192, 640, 4, 320, 1024, 192, 640, two, two) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "alias") != NULL);
    EXPECT(PREP(one, NULL, t, t, 192, 640, 4, 320, 1024, 192, 640, one, three) == DMH_EINVAL);
    EXPECT(PREP(one, NULL, t, t, 192, 640, 4, 320, 1024, 192, 640, two, one) == DMH_EINVAL);
    if (failures) {
        fprintf(stderr, "hint_checks: %d failure(s)\n", failures);
        return 1;
    }
    printf("hint_checks: ok\n");
    return 0;
}
