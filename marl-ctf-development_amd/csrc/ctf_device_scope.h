// ctf_device_scope.h — the library's one way of switching devices (host only): every entry point of both C ABIs that works on a
// device other than the caller's current one declares a DeviceScope and leaves through any `return` it likes.
#pragma once
#include <hip/hip_runtime.h>

// makes `want` current for the lifetime of the object, then puts the caller's device back
struct DeviceScope {
    int prev = -1, want;
    const char* error = nullptr;  // the call that failed (nothing was switched then), or NULL
    explicit DeviceScope(int device_id) : want(device_id) {
        if (hipGetDevice(&prev) != hipSuccess) error = "hipGetDevice failed";
        else if (prev != want && hipSetDevice(want) != hipSuccess) error = "hipSetDevice failed";
    }
    ~DeviceScope() {
        if (!error && prev != want) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};
