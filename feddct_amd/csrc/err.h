// err.h — the library's error slot, for units with and without HIP.
#pragma once

namespace fa {
// thread-local last-error message (fa_last_error); returns code
int set_err(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
}  // namespace fa
