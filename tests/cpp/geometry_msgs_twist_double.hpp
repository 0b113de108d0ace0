// geometry_msgs_twist_double.hpp -- a test double of the members of geometry_msgs::Twist that include/ssf.hpp's fillTwist fills
// (geometry_msgs/Twist.msg, geometry_msgs/Vector3.msg): linear and angular.  Field types as the ROS message generator emits them.
// Test infrastructure only: a node includes <geometry_msgs/Twist.h> instead.
#pragma once
namespace geometry_msgs {
struct Vector3 { double x, y, z; };
struct Twist { Vector3 linear, angular; };
}  // namespace geometry_msgs
