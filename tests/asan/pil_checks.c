/* Host side of K31's entry points (dmh_pil_resample_tables_size, dmh_pil_resample) under AddressSanitizer, as
 * tests/asan/host_checks.c does it for the rest of the library: linked against libdmh_hip_asan.so (host code only, no device
 * code).  Table sizes against Pillow's ksize arithmetic, every argument check, and the NULL-output forms: each launch call
 * below must be refused on the host before any launch.  Compiled as C.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "dmh_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            fprintf(stderr, "pil_checks: %s (line %d): %s\n", #cond, __LINE__, dmh_last_error()); \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

int main(void) {
    void* one = (void*)(uintptr_t)64;       /* a non-NULL, 4-byte aligned dummy "device pointer" */
    void* odd = (void*)(uintptr_t)66;
    const int32_t* t = (const int32_t*)one;

    /* table sizes: out * (2 + ksize), ksize = 2 ceil(support * max(in / out, 1)) + 1; an unchanged size is (x, 1, 2^22) */
    EXPECT(dmh_pil_resample_tables_size(1242, 1024, DMH_PIL_LANCZOS) == 1024 * (2 + 9));
    EXPECT(dmh_pil_resample_tables_size(375, 320, DMH_PIL_LANCZOS) == 320 * (2 + 9));
    EXPECT(dmh_pil_resample_tables_size(320, 160, DMH_PIL_LANCZOS) == 160 * (2 + 13));
    EXPECT(dmh_pil_resample_tables_size(370, 375, DMH_PIL_LANCZOS) == 375 * (2 + 7));
    EXPECT(dmh_pil_resample_tables_size(7, 13, DMH_PIL_BILINEAR) == 13 * (2 + 3));
    EXPECT(dmh_pil_resample_tables_size(123, 96, DMH_PIL_BILINEAR) == 96 * (2 + 5));
    EXPECT(dmh_pil_resample_tables_size(96, 96, DMH_PIL_LANCZOS) == 96 * 3);
    EXPECT(dmh_pil_resample_tables_size(0, 96, DMH_PIL_LANCZOS) == -1);
    EXPECT(dmh_pil_resample_tables_size(96, 0, DMH_PIL_LANCZOS) == -1);
    EXPECT(dmh_pil_resample_tables_size(96, 48, 0) == -1 && dmh_pil_resample_tables_size(96, 48, 3) == -1);
    EXPECT(dmh_pil_resample_tables_size(1 << 20, 48, DMH_PIL_LANCZOS) == -1);
    for (int in = 1; in < 400; in += 7)
        for (int out = 1; out < 400; out += 11) EXPECT(dmh_pil_resample_tables_size(in, out, DMH_PIL_LANCZOS) >= 3 * out);

    /* a good call's arguments, each broken in turn (uint8 HWC 38 x 124 x 3 -> 32 x 96) */
#define CALL(src, f32, sn, sc, sy, sx, Hs, Ws, tab, words, desc, flip, N, C, Ho, Wo, rows, o8, of) \
    dmh_pil_resample(src, f32, sn, sc, sy, sx, Hs, Ws, tab, words, desc, flip, N, C, Ho, Wo, rows, (uint8_t*)(o8), (float*)(of), NULL)
    EXPECT(CALL(NULL, 0, 14136, 1, 372, 3, 38, 124, t, 2000, t, NULL, 2, 3, 32, 96, 17, one, one) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "null pointer") != NULL);
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, NULL, 2000, t, NULL, 2, 3, 32, 96, 17, one, one) == DMH_EINVAL);
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, t, 2000, NULL, NULL, 2, 3, 32, 96, 17, one, one) == DMH_EINVAL);
    /* the NULL-output forms: either output may be missing, not both */
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, t, 2000, t, NULL, 2, 3, 32, 96, 17, NULL, NULL) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "out_u8 or out_f32") != NULL);
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, t, 2000, t, NULL, 0, 3, 32, 96, 17, one, NULL) == DMH_EINVAL);
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, t, 2000, t, NULL, 2, 3, 0, 96, 17, NULL, one) == DMH_EINVAL);
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, t, 2000, t, NULL, 65536, 3, 32, 96, 17, one, NULL) == DMH_EINVAL);
    EXPECT(CALL(one, 0, 14136, 1, 0, 3, 38, 124, t, 2000, t, NULL, 2, 3, 32, 96, 17, one, NULL) == DMH_EINVAL);
    EXPECT(CALL(one, 0, -1, 1, 372, 3, 38, 124, t, 2000, t, NULL, 2, 3, 32, 96, 17, one, NULL) == DMH_EINVAL);
    EXPECT(CALL(one, 0, (int64_t)1 << 31, 1, 372, 3, 38, 124, t, 2000, t, NULL, 2, 3, 32, 96, 17, one, NULL) == DMH_EINVAL);
    EXPECT(strstr(dmh_last_error(), "2^31") != NULL);
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, t, 2000, t, NULL, 2, 3, 1 << 15, 1 << 15, 1, one, NULL) == DMH_EINVAL);
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, t, 0, t, NULL, 2, 3, 32, 96, 17, one, NULL) == DMH_EINVAL);
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, t, (int64_t)1 << 31, t, NULL, 2, 3, 32, 96, 17, one, NULL) == DMH_EINVAL);
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, t, 2000, t, NULL, 2, 3, 32, 96, 0, one, NULL) == DMH_EINVAL);
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, t, 2000, t, NULL, 2, 3, 32, 96, 683, one, NULL) == DMH_EINVAL);   /* 683 x 96 > 64 KiB */
    EXPECT(strstr(dmh_last_error(), "lds_rows") != NULL);
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, (const int32_t*)odd, 2000, t, NULL, 2, 3, 32, 96, 17, one, NULL) == DMH_EINVAL);
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, t, 2000, t, (const int32_t*)odd, 2, 3, 32, 96, 17, one, NULL) == DMH_EINVAL);
    EXPECT(CALL(odd, 1, 14136, 4712, 124, 1, 38, 124, t, 2000, t, NULL, 2, 3, 32, 96, 17, one, NULL) == DMH_EINVAL);  /* float source */
    EXPECT(CALL(odd, 0, 14136, 1, 372, 3, 38, 124, t, 2000, t, NULL, 2, 3, 32, 96, 17, odd, NULL) == DMH_EINVAL);     /* out aliases src */
    EXPECT(CALL(one, 0, 14136, 1, 372, 3, 38, 124, t, 2000, t, NULL, 2, 3, 32, 96, 17, NULL, odd) == DMH_EINVAL);     /* float out */
    if (failures) {
        fprintf(stderr, "pil_checks: %d failure(s)\n", failures);
        return 1;
    }
    printf("pil_checks: ok\n");
    return 0;
}
