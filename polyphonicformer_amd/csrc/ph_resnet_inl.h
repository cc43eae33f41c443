// What the backbone's inference kernels (ph_resnet.hip) and its training kernels (ph_resnet_train.hip) share: the tile constants of the
// channels-last implicit GEMM, the one geometry rule and the one argument check.
#pragma once
#include "ph_common.h"

constexpr int RC_THREADS = 256;
constexpr int RC_KC = 64;                // input channels per chunk
constexpr int RC_LDA = RC_KC + 8;        // row pitch of the staged chunk, 16-bit elements (144 bytes: 16-byte aligned rows)

// geometry of one layer: 0 = 64 x 64, 1 = 128 x 64, 2 = 128 x 128 (pixels x channels per workgroup).  A function of the layer's
// shape only, never of B.  The wide forms need enough tiles per frame to fill the 256 CUs; below that the small tile has less
// tail and more workgroups.
static inline int rc_geometry(int64_t HoWo, int Cout) {
    const int64_t t128 = (HoWo + 127) / 128;
    if (Cout % 128 == 0 && t128 * (Cout / 128) >= 256) return 2;
    if (t128 * (Cout / 64) >= 256) return 1;
    return 0;
}

static inline int rc_check(const char* fn, int ksize, int stride, int Cin, int Cout, int H, int W, int B) {
    PH_CHECK_ARG_AS(fn, ksize == 1 || ksize == 3, "ksize must be 1 or 3");
    PH_CHECK_ARG_AS(fn, stride == 1 || stride == 2, "stride must be 1 or 2");
    PH_CHECK_ARG_AS(fn, Cin >= 64 && Cin <= 2048 && Cin % 64 == 0, "Cin must be a multiple of 64 in [64, 2048]");
    PH_CHECK_ARG_AS(fn, Cout >= 64 && Cout <= 2048 && Cout % 64 == 0, "Cout must be a multiple of 64 in [64, 2048]");
    PH_CHECK_ARG_AS(fn, B > 0 && B <= 65535 && H > 0 && W > 0 && H <= 32768 && W <= 32768, "B, H, W out of range");
    return PH_OK;
}
