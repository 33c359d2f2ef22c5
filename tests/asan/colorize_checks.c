/* Host side of K37's entry points (dmh_disp_colorize, dmh_disp_colorize_ws_size) under AddressSanitizer, as tests/asan/hint_checks.c
 * does it for K34: linked against libdmh_hip_asan.so (host code only, no device code).  Every argument check: each call below must
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
            fprintf(stderr, "colorize_checks: %s (line %d): %s\n", #cond, __LINE__, dmh_last_error()); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

int main(void) {
    void* one = (void*)(uintptr_t)64;       /* non-NULL, aligned dummy "device pointers" */
    void* two = (void*)(uintptr_t)128;
    void* by2 = (void*)(uintptr_t)66;       /* 2-byte aligned only */
    const float* src = (const float*)one;
    const uint8_t* tab = (const uint8_t*)(uintptr_t)65;    /* bytes need no alignment */
    uint8_t* out = (uint8_t*)(uintptr_t)67;
    /* a good call: 4 maps of 192 x 640, 6 panels of 375 x 1242 side by side in two rows of three */
    enum { P = 6, H = 375, W = 1242 };
    const int64_t pitch = 3 * 3 * W, len = 2 * H * pitch;
    dmh_colorize_panel good[DMH_COLORIZE_MAX_PANELS + 1], p[DMH_COLORIZE_MAX_PANELS + 1];
    memset(good, 0, sizeof(good));
    for (int i = 0; i < DMH_COLORIZE_MAX_PANELS + 1; ++i) {
        good[i].a = i % 4;
        good[i].b = i % 3 == 2 ? (i + 1) % 4 : -1;
        good[i].mode = i % 3;
        good[i].ref = 0;
        good[i].origin = i < P ? (int64_t)(i / 3) * H * pitch + (int64_t)(i % 3) * 3 * W : 0;
    }
#define CALL(src, ns, h, w, pn, np, HH, WW, lo, hi, g, tab, map, ws, st, out, len, pitch) \
    dmh_disp_colorize(src, ns, h, w, pn, np, HH, WW, lo, hi, g, tab, (float*)(map), (uint32_t*)(ws), (float*)(st), out, len, pitch, NULL)
#define RESET() memcpy(p, good, sizeof(good))
    const int lo = 442461, hi = 442462;
    const float g = 0.25f;

    EXPECT(DMH_COLORIZE_MAX_PANELS == 32 && DMH_COLORIZE_STATS == 5 && sizeof(dmh_colorize_panel) == 24);
    EXPECT(dmh_disp_colorize_ws_size(1) == 3 * 2 * 2048 + 8);
    EXPECT(dmh_disp_colorize_ws_size(32) == 32 * (3 * 2 * 2048 + 8));
    EXPECT(dmh_disp_colorize_ws_size(0) == -1 && dmh_disp_colorize_ws_size(-4) == -1 && dmh_disp_colorize_ws_size(33) == -1);

    RESET();
    /* null pointers */
    EXPECT(CALL(NULL, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "null pointer") != NULL);
    EXPECT(CALL(src, 4, 192, 640, NULL, P, H, W, lo, hi, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, NULL, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, NULL, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, NULL, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, one, NULL, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, one, one, NULL, len, pitch) == DMH_EINVAL);
    /* shapes */
    EXPECT(CALL(src, 0, 192, 640, p, P, H, W, lo, hi, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "B, h, w >= 1") != NULL);
    EXPECT(CALL(src, 4, 0, 640, p, P, H, W, lo, hi, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, -1, p, P, H, W, lo, hi, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 40000, 40000, p, P, H, W, lo, hi, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "2^31") != NULL);
    EXPECT(CALL(src, 4, 192, 640, p, P, 0, W, 0, 0, 0.f, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "H, W >= 1") != NULL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, 0, 0, 0, 0.f, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, -H, W, 0, 0, 0.f, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, 20000, 20000, 0, 0, 0.f, tab, one, one, one, out, (int64_t)1 << 40, 60000) == DMH_EINVAL);
    /* the panel count */
    EXPECT(CALL(src, 4, 192, 640, p, 0, H, W, lo, hi, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "DMH_COLORIZE_MAX_PANELS") != NULL);
    EXPECT(CALL(src, 4, 192, 640, p, -1, H, W, lo, hi, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, DMH_COLORIZE_MAX_PANELS + 1, 2, 2, 2, 3, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    /* the percentile plan */
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, -1, 0, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "ranks") != NULL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, H * W, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, H * W, H * W, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, hi, lo, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, lo + 2, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, 1.f, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "weight") != NULL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, -0.5f, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, 0.f / 0.f, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    /* alignment */
    EXPECT(CALL((const float*)by2, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "aligned") != NULL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, by2, one, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, by2, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, one, by2, out, len, pitch) == DMH_EINVAL);
    /* the output's pitch and length */
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, len, 3 * W - 1) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "pitch") != NULL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, 0, pitch) == DMH_EINVAL);
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, len - 1, pitch) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "inside the output") != NULL);
    /* the records: maps outside the batch */
    RESET(); p[3].a = 4;
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "lie in the batch") != NULL);
    RESET(); p[0].a = -1;
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, len, pitch) == DMH_EINVAL);
    RESET(); p[5].b = 4;
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, len, pitch) == DMH_EINVAL);
    RESET(); p[5].b = -2;
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, len, pitch) == DMH_EINVAL);
    /* a bad mode word */
    RESET(); p[2].mode = 3;
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "bad mode word") != NULL);
    RESET(); p[2].mode = -1;
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, len, pitch) == DMH_EINVAL);
    /* a limit record that names a panel outside the batch (only where the mode reads it) */
    RESET(); p[1].ref = P;
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "outside the batch") != NULL);
    RESET(); p[4].ref = -1;
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, len, pitch) == DMH_EINVAL);
    /* origins */
    RESET(); p[0].origin = -3;
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, len, pitch) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "inside the output") != NULL);
    RESET(); p[5].origin += 3;
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, len, pitch) == DMH_EINVAL);
    RESET(); p[5].origin = INT64_MAX - 8;
    EXPECT(CALL(src, 4, 192, 640, p, P, H, W, lo, hi, g, tab, one, two, one, out, len, pitch) == DMH_EINVAL);
    if (failures) {
        fprintf(stderr, "colorize_checks: %d failure(s)\n", failures);
        return 1;
    }
    printf("colorize_checks: ok\n");
    return 0;
}
