// The five batch gathers with fp32 outputs (the fp32 executor's input and target buffers,
// Cpad = Cin): element-type independent, built once (gather.h, gather_resample.h; the shape
// check: gather.hip).
#include "gather_resample.h"

namespace unet {

hipError_t f32_gather_launch(GatherOp op, const GatherArgs& a, void* xb, void* tb, hipStream_t s) {
  return gather_launch_t<float>(op, a, (float*)xb, (float*)tb, s);
}

}  // namespace unet
