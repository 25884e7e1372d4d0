/* Stand-in for Boost.Python: just enough for simulator_entity.h and simulator.h to compile.  Nothing on the SimpleGame /
 * SimpleRace path calls it; every use aborts. */
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>

namespace boost {
namespace python {
inline void xwref_never() {
    std::fprintf(stderr, "boost::python stand-in called\n");
    std::abort();
}
class object {
  public:
    object() {}
    template <typename T>
    object(const T&) { xwref_never(); }
    template <typename T>
    object operator[](const T&) const { xwref_never(); return object(); }
};
class dict : public object {};
class tuple : public object {};
template <typename T>
class extract {
  public:
    extract(const object&) { xwref_never(); }
    operator T() const { return T(); }
};
template <typename... A>
tuple make_tuple(const A&...) { xwref_never(); return tuple(); }
}  // namespace python
}  // namespace boost
