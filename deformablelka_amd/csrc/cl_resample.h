// The launch counter of the resampling entries (dlka_resample_launch_count, include/dlka.h), defined in cl_resample.hip.  cl_spline.hip's
// entries count here too: the pad and the prefilter were resampling entries before the augmentation and the 2-D evaluator shared them.
#pragma once
#include "cl_pipeline.h"

namespace dlka {
extern LaunchCounter g_rs_launches;
}
