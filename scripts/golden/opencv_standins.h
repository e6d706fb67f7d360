// Force-included in front of the LDSO sources' FeatureDetector.cc when it is compiled for scripts/golden/make_ref_detect_corners.py: the OpenCV names that file
// uses (rounding helpers, CV_PI, and empty stand-ins for the drawing calls of DrawFeatures, which is never called).
#pragma once
#include <cmath>
static inline int cvFloor(double v) { return (int) std::floor(v); }
static inline int cvCeil(double v) { return (int) std::ceil(v); }
static inline int cvRound(double v) { return (int) std::lrint(v); }
#define CV_PI 3.1415926535897932384626433832795
#define CV_8UC3 16
typedef unsigned char uchar;
namespace cv {
struct Point2f { Point2f(float, float) {} };
struct Scalar { Scalar(int, int, int) {} };
template <class M> inline void circle(M &, Point2f, int, Scalar, int) {}
template <class S, class M> inline void imshow(const S &, M &) {}
inline int waitKey(int) { return 0; }
}
