// failf.h -- the declaration of failf alone, for host code that must compile without the HIP
// runtime headers (system_stage.h); everything else includes it through last_error.h.
#pragma once

namespace ol {

// store the formatted message as the text ol_last_error() returns on this thread; returns `code`
int failf(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

}  // namespace ol
