// light_math.h — the arithmetic of an area light's cdf entry, for BOTH sides: the host library (g++: the upload's light section and
// yh_triangle_cdf) and the device (hipcc, unit/light_list.hip: the light list made again by an edit). One text, the reference's operation
// order (triangle_area, math.h:3306), IEEE square root on both sides and no contracted multiply-add on either (unit/object_math.h), so
// both give the same bits. The SUM of the entries is not here: it is one float chain in element order, which each side runs itself.
#ifndef YH_LIGHT_MATH_H_
#define YH_LIGHT_MATH_H_
#include <math.h>

#include "object_math.h"

namespace {

YH_HD float triangle_area(F3 p0, F3 p1, F3 p2) {
  F3 c = cross(p1 - p0, p2 - p0);
  return sqrtf(dot(c, c)) / 2;
}

}  // namespace
#endif
