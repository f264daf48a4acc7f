// ref_std_math.h -- TEST INFRASTRUCTURE ONLY.
//
// Forced into the in-place compile of the reference's camera.cc and
// voxel_octree.cc (oracle/Makefile, _ref/libvrtref_gi.so).  The reference
// spells the C float math functions std::tanf, std::sqrtf, ... as MSVC's
// <cmath> allows; libstdc++ declares them in the global namespace only.  This
// header names the same C library functions in namespace std.  No arithmetic.
#ifndef VRT_REF_STD_MATH_H
#define VRT_REF_STD_MATH_H
#include <cmath>
namespace std
{
using ::acosf;
using ::asinf;
using ::atan2f;
using ::atanf;
using ::ceilf;
using ::cosf;
using ::expf;
using ::fabsf;
using ::floorf;
using ::fmodf;
using ::log2f;
using ::logf;
using ::powf;
using ::sinf;
using ::sqrtf;
using ::tanf;
}
#endif
