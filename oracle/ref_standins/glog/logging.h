/* Stand-in for glog.  LOG(INFO / WARNING / ERROR) and VLOG discard their text; LOG(FATAL) and a failed CHECK* print the
 * message and abort, as glog does -- a failed check never passes silently.  The macros yield a std::ostream& like glog's, so
 * operator<< overloads are looked up at the call site. */
#pragma once
#include <gflags/gflags.h>
#include <cstdio>
#include <cstdlib>
#include <functional>   /* real glog pulls these in; simulator_util.h relies on it */
#include <iostream>
#include <sstream>
#include <string>

namespace xwref_glog {
class Sink {
  public:
    Sink(bool fatal, const char* file, int line, const char* what) : fatal_(fatal) {
        if (fatal_) os_ << file << ":" << line << "] " << what;
    }
    ~Sink() {
        if (fatal_) {
            std::fprintf(stderr, "%s\n", os_.str().c_str());
            std::fflush(stderr);
            std::abort();
        }
    }
    std::ostream& stream() { return os_; }

  private:
    bool fatal_;
    std::ostringstream os_;
};
struct Voidify {
    void operator&(std::ostream&) {}
};
enum { FATAL_INFO = 0, FATAL_WARNING = 0, FATAL_ERROR = 0, FATAL_FATAL = 1 };
}  // namespace xwref_glog

#define LOG(severity) xwref_glog::Sink(xwref_glog::FATAL_##severity != 0, __FILE__, __LINE__, "").stream()
#define VLOG(level) true ? (void)0 : xwref_glog::Voidify() & xwref_glog::Sink(false, __FILE__, __LINE__, "").stream()
#define CHECK(cond) \
    (cond) ? (void)0 : xwref_glog::Voidify() & xwref_glog::Sink(true, __FILE__, __LINE__, "Check failed: " #cond " ").stream()
#define XWREF_CHECK_OP(a, b, op) CHECK((a) op (b))
#define CHECK_EQ(a, b) XWREF_CHECK_OP(a, b, ==)
#define CHECK_NE(a, b) XWREF_CHECK_OP(a, b, !=)
#define CHECK_LT(a, b) XWREF_CHECK_OP(a, b, <)
#define CHECK_LE(a, b) XWREF_CHECK_OP(a, b, <=)
#define CHECK_GT(a, b) XWREF_CHECK_OP(a, b, >)
#define CHECK_GE(a, b) XWREF_CHECK_OP(a, b, >=)
