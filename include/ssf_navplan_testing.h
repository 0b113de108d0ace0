/*
 * ssf_navplan_testing.h -- test and measurement hooks of ssf_navplan_field (ssf_navplan.h), exported next to it.  Not part of
 * the drop-in surface, and not in ssf_testing.h: that header lists what BOTH the product and the CPU oracle export, and the
 * oracle has no plan.
 */
#ifndef SSF_NAVPLAN_TESTING_H
#define SSF_NAVPLAN_TESTING_H
#include "ssf.h"
#ifdef __cplusplus
extern "C" {
#endif
/* the relaxation rounds launched between two reads of the flagged-tile count by the handle's later plans, 1..1024; 0 = the
   default.  Results never depend on it. */
int ssf_debug_navplan_set_round_batch(ssf_handle* h, int rounds);
/* what the handle's last ssf_navplan_field did: the rounds in which a tile was worked on, and the (round, tile) pairs */
int ssf_debug_navplan_last(const ssf_handle* h, int64_t* rounds, int64_t* tile_visits);
#ifdef __cplusplus
}
#endif
#endif /* SSF_NAVPLAN_TESTING_H */
