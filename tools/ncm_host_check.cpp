// Host-side size and argument checks of include/cse_ncm.h, as a stand-alone
// program for a sanitizer build (no device is needed: every call here is
// answered before any device work):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude \
//       -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       tools/ncm_host_check.cpp classical_speech_enhancement_amd/csrc/cse_ncm.hip \
//       -x hip classical_speech_enhancement_amd/csrc/cse_error.cpp -o ncm_host_check
//   ./ncm_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "cse_ncm.h"

static int failures = 0;

#define EXPECT(cond)                                               \
    do {                                                           \
        if (!(cond)) {                                             \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);  \
            ++failures;                                            \
        }                                                          \
    } while (0)

int main() {
    // sizes: 10 s at 16 kHz is e[J][25] and dx[M][25] as f64 and little else
    const int64_t J = 160000 / 120 - 4, M = (J - 8) / 4 + 1;
    const int64_t n = cse_ncm_workspace_bytes(1, 160000, 16000);
    EXPECT(n >= (J + M) * 25 * 8 && n < (J + M) * 25 * 8 + 4096);
    EXPECT(cse_ncm_workspace_bytes(1, 160000, 16000) * 3 <=
           cse_ncm_workspace_bytes(3, 160000, 16000) + 3 * 1280);
    EXPECT(cse_ncm_workspace_bytes(1, 479, 16000) >= 0);    // J = 0
    EXPECT(cse_ncm_workspace_bytes(1, 1800, 16000) >= 0);   // J = 11: no score
    EXPECT(cse_ncm_workspace_bytes(0, 0, 8000) >= 0);
    EXPECT(cse_ncm_workspace_bytes(1, 4000, 44100) == -1);
    EXPECT(cse_ncm_workspace_bytes(-1, 4000, 16000) == -1);
    EXPECT(cse_ncm_workspace_bytes(1, -1, 16000) == -1);
    // the largest sizes the entry points accept do not overflow
    EXPECT(cse_ncm_workspace_bytes(65535, ((int64_t)1 << 36) - 1, 8000) > 0);
    EXPECT(cse_ncm_workspace_bytes(65536, 4000, 16000) == -1);
    EXPECT(cse_ncm_workspace_bytes(1, (int64_t)1 << 36, 16000) == -1);
    EXPECT(cse_ncm_workspace_bytes(INT64_MAX, INT64_MAX, 16000) == -1);
    EXPECT(cse_ncm_scratch_bytes(4096, 160000, 16000) == 0);
    EXPECT(cse_ncm_scratch_bytes(INT64_MAX, INT64_MAX, 8000) == 0);
    EXPECT(cse_ncm_scratch_bytes(-1, 4000, 16000) == -1);
    EXPECT(cse_ncm_scratch_bytes(1, -1, 16000) == -1);
    EXPECT(cse_ncm_scratch_bytes(1, 4000, 0) == -1);

    // refused calls: the pointers are never read
    static double clean[8];
    static float y[8];
    static int64_t off[1];
    static int32_t sig[1];
    static unsigned char ws[8];
    static double out[2];
    EXPECT(cse_ncm_prepare(nullptr, 1, 4000, 16000, ws, nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_prepare(clean, 1, 4000, 16000, nullptr, nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_prepare(clean, 0, 4000, 16000, ws, nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_prepare(clean, -3, 4000, 16000, ws, nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_prepare(clean, 65536, 4000, 16000, ws, nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_prepare(clean, 1, 0, 16000, ws, nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_prepare(clean, 1, INT64_MAX, 16000, ws, nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_prepare(clean, 1, 4000, 22050, ws, nullptr) == CSE_EINVAL);
    EXPECT(std::strstr(cse_last_error(), "22050") != nullptr);
    // a clip without a score launches nothing and leaves the workspace alone
    EXPECT(cse_ncm_prepare(clean, 1, 1800, 16000, ws, nullptr) == CSE_OK);
    EXPECT(cse_ncm_cells(nullptr, off, nullptr, sig, 1, 1, 4000, 16000, 1, ws, nullptr, 1.0, out,
                         nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_cells(y, nullptr, nullptr, sig, 1, 1, 4000, 16000, 1, ws, nullptr, 1.0, out,
                         nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_cells(y, off, nullptr, nullptr, 1, 1, 4000, 16000, 1, ws, nullptr, 1.0, out,
                         nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_cells(y, off, nullptr, sig, 1, 1, 4000, 16000, 1, nullptr, nullptr, 1.0, out,
                         nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_cells(y, off, nullptr, sig, 1, 1, 4000, 16000, 1, ws, nullptr, 1.0, nullptr,
                         nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_cells(y, off, nullptr, sig, -1, 1, 4000, 16000, 1, ws, nullptr, 1.0, out,
                         nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_cells(y, off, nullptr, sig, (int64_t)1 << 31, 1, 4000, 16000, 1, ws, nullptr,
                         1.0, out, nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_cells(y, off, nullptr, sig, 1, 0, 4000, 16000, 1, ws, nullptr, 1.0, out,
                         nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_cells(y, off, nullptr, sig, 1, 1, 0, 16000, 1, ws, nullptr, 1.0, out,
                         nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_cells(y, off, nullptr, sig, 1, 1, 4000, 48000, 1, ws, nullptr, 1.0, out,
                         nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_cells(y, off, nullptr, sig, 1, 1, 4000, 16000, 1, ws, nullptr, -0.25, out,
                         nullptr) == CSE_EINVAL);
    EXPECT(std::strstr(cse_last_error(), "bif_power") != nullptr);
    EXPECT(cse_ncm_cells(y, off, nullptr, sig, 1, 1, 4000, 16000, 1, ws, nullptr, NAN, out,
                         nullptr) == CSE_EINVAL);
    EXPECT(cse_ncm_cells(y, off, nullptr, sig, 1, 1, 4000, 16000, 1, ws, nullptr, INFINITY, out,
                         nullptr) == CSE_EINVAL);
    EXPECT(std::strstr(cse_last_error(), "cse_ncm_cells") != nullptr);
    // n_cells == 0 launches nothing
    EXPECT(cse_ncm_cells(y, off, nullptr, sig, 0, 1, 4000, 16000, 1, ws, nullptr, 0.0, out,
                         nullptr) == CSE_OK);
    std::printf(failures ? "%d check(s) failed\n" : "ncm host checks: all passed\n", failures);
    return failures ? 1 : 0;
}
