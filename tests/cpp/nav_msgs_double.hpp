// nav_msgs_double.hpp -- a test double of the members of nav_msgs::OccupancyGrid that include/ssf.hpp's fillOccupancyGrid fills
// (nav_msgs/OccupancyGrid.msg, nav_msgs/MapMetaData.msg, geometry_msgs/Pose.msg): data, info.resolution, info.width,
// info.height, info.origin.  Field types as the ROS message generator emits them.
// Test infrastructure only: a node includes <nav_msgs/OccupancyGrid.h> instead.
#pragma once
#include <cstdint>
#include <vector>
namespace geometry_msgs {
struct Point { double x = 0, y = 0, z = 0; };
struct Quaternion { double x = 0, y = 0, z = 0, w = 0; };
struct Pose { Point position; Quaternion orientation; };
}  // namespace geometry_msgs
namespace nav_msgs {
struct MapMetaData { float resolution = 0; uint32_t width = 0, height = 0; geometry_msgs::Pose origin; };
struct OccupancyGrid { MapMetaData info; std::vector<int8_t> data; };
}  // namespace nav_msgs
