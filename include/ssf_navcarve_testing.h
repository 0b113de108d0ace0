/*
 * ssf_navcarve_testing.h -- test and measurement hooks of ssf_navgrid_carve (ssf_navcarve.h), exported next to it.  Not part of
 * the drop-in surface, and not in ssf_testing.h: that header lists what BOTH the product and the CPU oracle export, and the
 * oracle has no carve.
 */
#ifndef SSF_NAVCARVE_TESTING_H
#define SSF_NAVCARVE_TESTING_H
#include "ssf.h"
#ifdef __cplusplus
extern "C" {
#endif
/* the rays per chunk of the handle's later carves, 1 .. 2^24; 0 = the default 2^20.  Results do not depend on it. */
int ssf_debug_navcarve_set_chunk_rays(ssf_handle* h, int max_rays);
/* what the handle's last ssf_navgrid_carve did: its chunks, and the atomics it issued on `seen` (<= ray_entries) */
int ssf_debug_navcarve_last(const ssf_handle* h, int64_t* chunks, int64_t* atomics);
#ifdef __cplusplus
}
#endif
#endif /* SSF_NAVCARVE_TESTING_H */
