/* Stand-in for <opencv2/highgui/highgui.hpp>: windows, keys and image files do nothing. */
#pragma once
#include <opencv2/core/core.hpp>
#include <string>
#include <vector>

enum { CV_IMWRITE_PNG_COMPRESSION = 16 };
namespace cv {
enum { EVENT_LBUTTONDBLCLK = 7 };
inline void imshow(const std::string&, const Mat&) {}
inline int waitKey(int = 0) { return -1; }
inline bool imwrite(const std::string&, const Mat&, const std::vector<int>& = std::vector<int>()) { return true; }
}  // namespace cv
