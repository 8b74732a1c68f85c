// trl_hd.h -- TRL_HD, in front of every rule that the kernels and the host test programs both run.  Plain C++, no HIP header: the
// test programs include the rule headers alone, and under hipcc a rule header may come before the runtime's (whose __forceinline__
// is this attribute).
#pragma once

#if defined(__HIPCC__)
#define TRL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TRL_HD inline
#endif
