/* Stand-in <math.h>, found before the C++ library's own wrapper of that name.
 *
 * The reference's simple_race_simulator.h includes <math.h> and then calls the unqualified cos / sin / floor / sqrt / acos /
 * fabs on floats.  On its 2017 toolchain those were the C library's double functions; the source only compiles that way
 * (std::min(1.0d, t.x * cos(a) + ...), std::min(floor(...), double(...)) need double results).  Today's libstdc++ <math.h>
 * adds `using std::cos;` etc., whose float overloads would win and the file is rejected.  <cmath> alone keeps the float
 * overloads inside namespace std and leaves glibc's C declarations as the only global ones. */
#include <cmath>
