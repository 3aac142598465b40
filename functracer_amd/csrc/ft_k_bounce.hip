#define FT_UNIT FT_UNIT_BOUNCE   // one of the three units libfunctracer_hip.so is linked from (ft_kernels.hip, "Translation units")
#include "ft_kernels.hip"
