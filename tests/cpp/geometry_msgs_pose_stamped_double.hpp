// geometry_msgs_pose_stamped_double.hpp -- a test double of the members of geometry_msgs::PoseStamped that include/ssf.hpp's
// fillExploreGoal fills (geometry_msgs/PoseStamped.msg): pose.position and pose.orientation.  A Path is a list of the same message,
// so the type is the one nav_msgs_path_double.hpp declares: a program may fill a Path and a goal side by side.
// Test infrastructure only: a node includes <geometry_msgs/PoseStamped.h> instead.
#pragma once
#include "nav_msgs_path_double.hpp"
