// cv_double_mask.hpp -- cv_double_u16.hpp with CV_8UC1 as well: include/ssf.hpp's cv::Mat overload with a pixel mask then exists.
// Test infrastructure only.
#pragma once
#define CV_8UC1 0
#include "cv_double_u16.hpp"
