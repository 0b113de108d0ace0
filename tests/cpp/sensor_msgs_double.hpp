// sensor_msgs_double.hpp -- a test double of the members of sensor_msgs::LaserScan that include/ssf.hpp's laserScan fills
// (sensor_msgs/LaserScan.msg): angle_min, angle_max, angle_increment, time_increment, scan_time, range_min, range_max, ranges,
// intensities.  Field types as the ROS message generator emits them.
// Test infrastructure only: a node includes <sensor_msgs/LaserScan.h> instead.
#pragma once
#include <vector>
namespace sensor_msgs {
struct LaserScan {
    float angle_min = 0, angle_max = 0, angle_increment = 0, time_increment = 0, scan_time = 0, range_min = 0, range_max = 0;
    std::vector<float> ranges, intensities;
};
}  // namespace sensor_msgs
