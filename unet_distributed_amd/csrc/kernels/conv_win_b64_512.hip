// Row-window conv kernels with 64-output-channel tiles and 512-pixel windows on 16 / 32 /
// 64-wide rows (conv_win.h win_b512_eligible; on 16-wide rows a window is two whole 16 x 16
// images), a translation unit of their own so the build compiles them beside
// conv_win_b64.hip, whose launch_win<64, 256> hands these convs over.
#define UNET_WIN_IMPL
#include "conv_win.h"

namespace unet {
template hipError_t launch_win<64, 512>(const ConvFwdParams&, hipStream_t);
}  // namespace unet
