// code_object.h -- which device symbols a built library file carries (code_object.cpp).
#pragma once
#include <string>
#include <vector>

// Sorted symbol names of every gfx950 code object in the clang offload bundles of the file at
// `path`.  File reads only (no HIP call); empty when the file cannot be read or holds none.
std::vector<std::string> slg_code_object_symbols(const char* path);
