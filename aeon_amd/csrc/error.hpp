// error.hpp -- the error a refused or failed call throws (stage.cpp's `guarded` turns it into the C ABI's
// code and aeon_hip_last_error's text); shared by the planner (plan.cpp) and the device half (stage.cpp).
#pragma once
#include <stdexcept>
#include <string>

namespace aeon_hip {

struct aeon_error : std::runtime_error {
    int code;
    aeon_error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
[[noreturn]] inline void fail(int code, const std::string& msg) { throw aeon_error(code, msg); }

} // namespace aeon_hip
