/* Stand-in for OpenCV 3.2 <opencv2/core/core.hpp>, as far as SimpleRace reads it.
 *
 * cv::Point_ arithmetic keeps the operand types of OpenCV 3.2's published core/types.hpp (the library is not on the build
 * machine, so this follows the header text and is not checked against a binary):
 *   Point + Point, Point - Point   saturate_cast<T>(a.x op b.x): float arithmetic for Point2f
 *   a += b                         a.x += b.x
 *   Point * float, float * Point   saturate_cast<T>(a.x * b) with b float: a float product
 *   Point * double, double * Point saturate_cast<T>(a.x * b) with b double: a double product narrowed once
 *   Point * int, int * Point       saturate_cast<T>(a.x * b)
 *   norm(Point_<T>)                std::sqrt((double)x * x + (double)y * y), a double
 * saturate_cast<float>(double) is a plain conversion.  Drawing is a no-op. */
#pragma once
#include <cmath>
#include <ostream>

namespace cv {

template <typename T>
class Point_ {
  public:
    Point_() : x(0), y(0) {}
    Point_(T _x, T _y) : x(_x), y(_y) {}
    template <typename T2>
    operator Point_<T2>() const { return Point_<T2>(static_cast<T2>(x), static_cast<T2>(y)); }
    T x, y;
};
typedef Point_<int> Point2i;
typedef Point_<float> Point2f;
typedef Point_<double> Point2d;
typedef Point2i Point;

template <typename T> inline Point_<T>& operator+=(Point_<T>& a, const Point_<T>& b) { a.x += b.x; a.y += b.y; return a; }
template <typename T> inline Point_<T>& operator-=(Point_<T>& a, const Point_<T>& b) { a.x -= b.x; a.y -= b.y; return a; }
template <typename T> inline Point_<T> operator+(const Point_<T>& a, const Point_<T>& b) {
    return Point_<T>(static_cast<T>(a.x + b.x), static_cast<T>(a.y + b.y));
}
template <typename T> inline Point_<T> operator-(const Point_<T>& a, const Point_<T>& b) {
    return Point_<T>(static_cast<T>(a.x - b.x), static_cast<T>(a.y - b.y));
}
template <typename T> inline Point_<T> operator*(const Point_<T>& a, int b) { return Point_<T>(static_cast<T>(a.x * b), static_cast<T>(a.y * b)); }
template <typename T> inline Point_<T> operator*(int a, const Point_<T>& b) { return Point_<T>(static_cast<T>(b.x * a), static_cast<T>(b.y * a)); }
template <typename T> inline Point_<T> operator*(const Point_<T>& a, float b) { return Point_<T>(static_cast<T>(a.x * b), static_cast<T>(a.y * b)); }
template <typename T> inline Point_<T> operator*(float a, const Point_<T>& b) { return Point_<T>(static_cast<T>(b.x * a), static_cast<T>(b.y * a)); }
template <typename T> inline Point_<T> operator*(const Point_<T>& a, double b) { return Point_<T>(static_cast<T>(a.x * b), static_cast<T>(a.y * b)); }
template <typename T> inline Point_<T> operator*(double a, const Point_<T>& b) { return Point_<T>(static_cast<T>(b.x * a), static_cast<T>(b.y * a)); }

template <typename T> inline double norm(const Point_<T>& pt) { return std::sqrt((double)pt.x * pt.x + (double)pt.y * pt.y); }

template <typename T> inline std::ostream& operator<<(std::ostream& os, const Point_<T>& p) { return os << "[" << p.x << ", " << p.y << "]"; }

class Scalar {
  public:
    Scalar(double a = 0, double b = 0, double c = 0, double d = 0) : val{a, b, c, d} {}
    double val[4];
};

class Mat {
  public:
    Mat() {}
    static Mat zeros(int, int, int) { return Mat(); }
};

}  // namespace cv

#define CV_8UC3 16
