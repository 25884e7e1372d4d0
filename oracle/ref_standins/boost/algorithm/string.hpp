/* Stand-in for <boost/algorithm/string.hpp>: boost::split with boost::is_any_of, token_compress_off behaviour
 * (adjacent separators give empty tokens; an empty input gives one empty token). */
#pragma once
#include <string>

namespace boost {
struct xwref_any_of {
    std::string set;
    bool operator()(char c) const { return set.find(c) != std::string::npos; }
};
inline xwref_any_of is_any_of(const std::string& s) { return xwref_any_of{s}; }

template <typename Seq, typename Pred>
Seq& split(Seq& out, const std::string& in, Pred pred) {
    out.clear();
    std::string cur;
    for (char c : in) {
        if (pred(c)) {
            out.push_back(cur);
            cur.clear();
        } else {
            cur += c;
        }
    }
    out.push_back(cur);
    return out;
}
}  // namespace boost
