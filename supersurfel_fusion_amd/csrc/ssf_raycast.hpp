// ssf_raycast.hpp -- what ssf_raycast.hip shares with the other read-outs that cast rays (ssf_navcarve.hip): the check of a call's
// parameters.  Private to the library's own files: nothing here is exported.
#pragma once
#include "ssf_handle.hpp"
#include "../../include/ssf_raycast.h"

#pragma GCC visibility push(hidden)
struct RaycastResolved { float tmin, tmax, s, cell; };      // the defaults resolved: cfg's range when both ends are 0, s 0 = 3, cell 0 = 0.125
// What ssf_raycast refuses of its parameters (include/ssf_raycast.h; rays, n and the outputs apart): the refusal's wording, or
// nullptr with r filled.  ONE copy of the rule: a caller that casts through ssf_raycast later refuses the same up front with it.
const char* raycast_params_refusal(const ssf_handle* h, const ssf_raycast_params* p, RaycastResolved& r);
#pragma GCC visibility pop
