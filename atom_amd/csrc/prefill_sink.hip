// The attention-sink instantiations of batch_prefill_kernel (prefill_i4.hip, kSink) as a translation unit of their own:
// prefill_i4.hip compiled again with only the kernel template and launch_prefill_sink() in it, so that these four kernels can be built
// without packed FP32 VALU ops (the Makefile's flag, as attn_d64.hip) while the older instantiations keep the code they have.
#define ATOM_PREFILL_SINK_TU
#include "prefill_i4.hip"
