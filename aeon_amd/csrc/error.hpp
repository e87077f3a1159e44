// error.hpp -- the errors a refused or failed call throws, and `guarded`, which turns them at the C ABI's
// boundary into the call's code and aeon_hip_last_error's text (the thread-local message itself lives in
// abi_host.cpp).  Shared by the planner (plan.cpp), the JPEG and PNG host code, and the entries of
// context.cpp, image_path.cpp, targets.cpp and abi_host.cpp.
#pragma once
#include <stdexcept>
#include <string>

#include "../../include/aeon_hip.h"

namespace aeon_hip {

struct aeon_error : std::runtime_error {
    int code;
    aeon_error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
[[noreturn]] inline void fail(int code, const std::string& msg) { throw aeon_error(code, msg); }

// Host-side error of the JPEG stage (and the PNG decoder), carrying its AEON_HIP_E* code across to the C ABI.
struct jpeg_error : std::runtime_error {
    int code;
    jpeg_error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// Sets the calling thread's aeon_hip_last_error text (abi_host.cpp).
void set_last_error(const char* what);

template <typename F>
int guarded(F&& f)
{
    try {
        return f();
    } catch (const aeon_error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const jpeg_error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::invalid_argument& e) {
        set_last_error(e.what());
        return AEON_HIP_EINVAL;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return AEON_HIP_ERUNTIME;
    }
}

} // namespace aeon_hip
