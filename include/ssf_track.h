/* ssf_track.h -- test hooks and counters of the HIP product's track stage that the CPU checker has no counterpart for (it runs no
 * launches): exported by the product library only, not part of ssf.h.
 *
 * The resident ICP launch: on a single shard, for a frame without a tile-sorted copy of its rows and a
 * configuration without the depth pre-filter in the frame (that pipeline is bound by its extract stage, not by tracking), the ICP
 * iterations and the association of a frame run in ONE launch whose workgroups keep their rows in registers and are sent one word
 * per iteration.  Results are the same bit for bit as with one launch per iteration. */
#ifndef SSF_TRACK_H
#define SSF_TRACK_H
#include "ssf.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Test hook (the companion of ssf_debug_set_bin_min_rows): up to how many visible rows a frame takes the resident launch.  Default
 * and ceiling 262 144 = 1024 workgroups, all of which must hold a place on the GPU at once: a safety condition, values above it
 * are clamped; 0 = never.  The ceiling assumes ONE handle tracking on the GPU: the resident grids of several handles add up, so
 * callers that share a GPU among handles with large maps lower it. */
int ssf_debug_set_resident_icp_max_rows(ssf_handle* h, int max_rows);
/* frames whose ICP iterations ran in a resident launch since the handle was created (the companion of ssf_waiter_matches, which
 * counts their association when the launch did it too) */
long long ssf_resident_icp_frames(ssf_handle* h);
/* ... and those of them whose launch started at its second word, because the frame's first record had been accumulated by the
 * frame before (pipelined frames, ssf_tuner_state [0] = 1) */
long long ssf_resident_icp_ahead_frames(ssf_handle* h);

#ifdef __cplusplus
}
#endif
#endif
