// hm_tie_slack.h -- the one piece of arithmetic the kernels (hm_common.h) and the host-only cut search (hm_cut_plan.h) share.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define HM_HOST_DEVICE_INLINE __host__ __device__ __forceinline__
#else
#define HM_HOST_DEVICE_INLINE inline
#endif

#define HM_TIE_SLACK 1024u         // ulps of u' that are treated as "may still order before" for u' >= 2 (see hm_tie_slack)

// How many ulps of u' above a key may still order BEFORE it by computed distance: d = acosh(u') / sqrt(c) is monotone in u' only
// up to the few-ulp error of acosh (2.5 ulps of d), so a pair at u' + s certainly has the larger d once the true increase
// s * ulp(u') / sqrt(u'^2 - 1) exceeds ~5 ulps of d.  For large u' (d ~ ln 2u') that takes up to 16 d ~ hundreds of ulps of u'
// -- HM_TIE_SLACK; near u' = 1 (d ~ sqrt(2 (u' - 1)), steep) a handful do: with t = u' - 1 < 1 the condition is s > ~20 t.
// 32 + 128 t is used below u' = 2.  (A constant 1024 made the exact top-1 search of a very dense table impossible: at d = 5,
// scale 0.01 there are ~10^5 pairs per ulp of u' -- round-3 fuzz.)  Non-decreasing in the bits.
HM_HOST_DEVICE_INLINE uint32_t hm_tie_slack(uint32_t ubits)
{
    if (ubits >= 0x40000000u) return HM_TIE_SLACK;
    return 32u + ((ubits > 0x3f800000u ? ubits - 0x3f800000u : 0u) >> 16);
}
