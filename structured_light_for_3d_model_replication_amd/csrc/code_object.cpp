// code_object.cpp -- reads the device symbol names out of a library file: every clang offload
// bundle in it ("__CLANG_OFFLOAD_BUNDLE__", entry table {offset, size, triple}), each gfx950 entry
// an ELF64 code object whose SHT_SYMTAB / SHT_DYNSYM tables are walked.  Host only, no HIP call.
// The file is untrusted input: every offset and size in it is a u64 of any value, so each range
// is checked as "length <= limit - offset" (never a sum that can wrap) before it is read, and a
// code object's ranges are confined to its own bundle entry.
#include "code_object.h"

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

namespace {

// [off, off + len) lies inside [0, lim)
bool fits(uint64_t off, uint64_t len, uint64_t lim) { return off <= lim && len <= lim - off; }

std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> b;
  FILE* f = path ? fopen(path, "rb") : nullptr;
  if (!f) return b;
  if (fseek(f, 0, SEEK_END) == 0) {
    const long n = ftell(f);
    if (n > 0 && fseek(f, 0, SEEK_SET) == 0) {
      b.resize(size_t(n));
      if (fread(b.data(), 1, b.size(), f) != b.size()) b.clear();
    }
  }
  fclose(f);
  return b;
}

template <class T>
T rd(const uint8_t* p) {
  T v;
  memcpy(&v, p, sizeof(T));
  return v;
}

// Names of one ELF64 code object, elf[0 .. len).
void elf_symbols(const uint8_t* elf, uint64_t len, std::vector<std::string>& names) {
  if (len < 64 || memcmp(elf, "\x7f" "ELF", 4) != 0) return;
  const uint64_t shoff = rd<uint64_t>(elf + 0x28);
  const uint16_t shentsize = rd<uint16_t>(elf + 0x3a), shnum = rd<uint16_t>(elf + 0x3c);
  if (shentsize < 64 || !fits(shoff, uint64_t(shnum) * shentsize, len)) return;
  for (uint16_t si = 0; si < shnum; ++si) {
    const uint8_t* sh = elf + shoff + uint64_t(si) * shentsize;
    const uint32_t type = rd<uint32_t>(sh + 4);
    if (type != 2 && type != 11) continue;   // SHT_SYMTAB, SHT_DYNSYM
    const uint64_t sym_off = rd<uint64_t>(sh + 24), sym_size = rd<uint64_t>(sh + 32), ent = rd<uint64_t>(sh + 56);
    const uint32_t link = rd<uint32_t>(sh + 40);
    if (ent < 24 || link >= shnum) continue;
    const uint8_t* strh = elf + shoff + uint64_t(link) * shentsize;
    const uint64_t str_off = rd<uint64_t>(strh + 24), str_size = rd<uint64_t>(strh + 32);
    if (!fits(sym_off, sym_size, len) || !fits(str_off, str_size, len)) continue;
    for (uint64_t q = 0; ent <= sym_size - q; q += ent) {   // q <= sym_size throughout
      const uint32_t nm = rd<uint32_t>(elf + sym_off + q);
      if (nm == 0 || nm >= str_size) continue;
      const char* c = reinterpret_cast<const char*>(elf + str_off + nm);
      names.emplace_back(c, strnlen(c, size_t(str_size - nm)));
    }
  }
}

}  // namespace

std::vector<std::string> slg_code_object_symbols(const char* path) {
  std::vector<std::string> names;
  const std::vector<uint8_t> b = read_file(path);
  const uint8_t* const p = b.data();
  const uint64_t n = b.size();
  static const char kMagic[] = "__CLANG_OFFLOAD_BUNDLE__";
  const uint64_t ml = sizeof(kMagic) - 1;
  for (uint64_t at = 0; fits(at, ml + 8, n); ++at) {
    if (p[at] != '_' || memcmp(p + at, kMagic, ml) != 0) continue;
    uint64_t e = at + ml;
    const uint64_t n_ent = rd<uint64_t>(p + e);
    e += 8;
    for (uint64_t k = 0; k < n_ent && fits(e, 24, n); ++k) {
      const uint64_t off = rd<uint64_t>(p + e), size = rd<uint64_t>(p + e + 8), tl = rd<uint64_t>(p + e + 16);
      e += 24;
      if (!fits(e, tl, n)) break;
      const std::string triple(reinterpret_cast<const char*>(p + e), size_t(tl));
      e += tl;
      // the entry, offsets from the bundle's start: an ELF64 code object
      if (triple.find("gfx950") != std::string::npos && fits(off, size, n - at)) elf_symbols(p + at + off, size, names);
    }
  }
  std::sort(names.begin(), names.end());
  return names;
}
