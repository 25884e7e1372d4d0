/* Stand-in for <opencv2/imgproc/imgproc.hpp>: every drawing call is a no-op. */
#pragma once
#include <opencv2/core/core.hpp>

namespace cv {
enum { FONT_HERSHEY_SIMPLEX = 0 };
template <typename... A> inline void circle(const A&...) {}
template <typename... A> inline void rectangle(const A&...) {}
template <typename... A> inline void line(const A&...) {}
template <typename... A> inline void arrowedLine(const A&...) {}
template <typename... A> inline void putText(const A&...) {}
}  // namespace cv
