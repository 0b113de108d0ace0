// nav_msgs_path_double.hpp -- a test double of the members of nav_msgs::Path that include/ssf.hpp's fillPath fills
// (nav_msgs/Path.msg, geometry_msgs/PoseStamped.msg): poses[i].pose.  The pose's own types are those of nav_msgs_double.hpp, so
// that a program may fill an OccupancyGrid and a Path side by side.  Field types as the ROS message generator emits them.
// Test infrastructure only: a node includes <nav_msgs/Path.h> instead.
#pragma once
#include <vector>
#include "nav_msgs_double.hpp"
namespace geometry_msgs {
struct PoseStamped { Pose pose; };
}  // namespace geometry_msgs
namespace nav_msgs {
struct Path { std::vector<geometry_msgs::PoseStamped> poses; };
}  // namespace nav_msgs
