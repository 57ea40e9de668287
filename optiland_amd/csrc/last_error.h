// last_error.h -- the library's one thread-local error message (ol_last_error), for the
// translation units other than capi.hip.  Defined in capi.hip; capi.hip itself references no
// symbol of the other units (tests/hostmath links it alone).
#pragma once

namespace ol {

// store `message` as the text ol_last_error() returns on this thread; returns `code`
int set_last_error(int code, const char* message);

}  // namespace ol
