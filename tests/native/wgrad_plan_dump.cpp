// Prints the weight-gradient planner's decisions (csrc/kernels/wgrad_plan.cpp) for queries read from
// stdin, one per line; tests/test_wgrad_plan.py compares the output with tests/data/wgrad_plans.txt.
//
//   route N H W Cin Cout kh kw ph pw stride
//       -> route=<library|square|rect> [variant= kernel= splits= kps= ws= cap=]
//   plan <square|rect> <variant> <splits> N H W Cin Cout kh kw ph pw stride
//       -> variant= kernel= splits= kps= ws=   |   error: <the refusal>
//   auto N H W Cin Cout kh kw ph pw stride        (conv_wgrad_rows_rect_auto)
//       -> variant=
// Each output line is the query followed by " -> " and the answer; '#' lines and empty lines are skipped.
#include "wgrad_plan.hpp"

#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>

using namespace kfk;

static bool read_shape(std::istream &in, WgradShape &s) {
    return static_cast<bool>(in >> s.N >> s.H >> s.W >> s.Cin >> s.Cout >> s.kh >> s.kw >> s.ph >> s.pw >> s.stride);
}

static std::string show(const WgradPlan &p) {
    std::ostringstream o;
    o << "variant=" << p.variant << " kernel=" << wgrad_kernel_name(p.kernel) << " splits=" << p.splits
      << " kps=" << p.kps << " ws=" << p.ws_floats;
    return o.str();
}

int main() {
    std::string line;
    int bad = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        const std::string query = line.substr(0, line.find(" -> "));
        std::istringstream in(query);
        std::string what;
        in >> what;
        WgradShape s{};
        std::cout << query << " -> ";
        try {
            if (what == "route" && read_shape(in, s)) {
                const WgradRouting r = conv_wgrad_route(s);
                std::cout << "route=" << wgrad_route_name(r.route);
                if (r.route != WgradRoute::Library) {
                    const WgradFamily f = r.route == WgradRoute::Square ? WgradFamily::Square : WgradFamily::Rect;
                    std::cout << " " << show(conv_wgrad_plan(s, f, r.variant)) << " cap=" << r.max_pixels;
                }
            } else if (what == "plan") {
                std::string family;
                int variant = 0, splits = 0;
                if (!(in >> family >> variant >> splits) || !read_shape(in, s)) throw std::runtime_error("bad query");
                std::cout << show(conv_wgrad_plan(s, family == "square" ? WgradFamily::Square : WgradFamily::Rect, variant, splits));
            } else if (what == "auto" && read_shape(in, s)) {
                std::cout << "variant=" << conv_wgrad_rows_rect_auto(s);
            } else {
                throw std::runtime_error("bad query");
            }
        } catch (const std::invalid_argument &e) {
            std::cout << "error: " << e.what();
        } catch (const std::runtime_error &e) {
            std::cout << "error: " << e.what();
            ++bad;
        }
        std::cout << "\n";
    }
    return bad ? 2 : 0;
}
