// like_program.h — a SQL LIKE pattern compiled into the segment program ah_string_like takes (include/arrowhip.h).  Header-only and
// free of the rest of the host layer, so that a stand-alone program can include it.
//
// Rules: Arrow C++'s match_like, as pyarrow 25 answers.  `%` any run of bytes, `_` one character, `\` makes the next pattern
// character literal whatever it is; the whole row must match.  Two things Arrow does that one would not guess, both kept:
//   * a pattern of the shape `%lit%`, `lit%` or `%lit` — lit without `%` and `_`, and for the first two shapes not ending in `\` —
//     is answered by Arrow's substring / prefix / suffix matchers with lit taken RAW: a `\` inside it is a literal backslash
//     (`%a\bc%` finds `a\bc`, not `abc`; `%a\` is "ends with a\").  Every other pattern has its escapes resolved (`a\bc` is `abc`);
//   * a lone `\` at the end of such a pattern is dropped: `a\` is the pattern `a`.
// The program: byte 0 flags (1: the first segment starts the row, 2: the last segment ends it), bytes 1-2 the number of segments,
// then per segment a 2-byte element count and {0, byte} (a literal byte) or {1, 0} (one character) per element.  Segments are what
// `%` separates; adjacent `%` are one; only a pattern without any `%` and without any character has an empty segment.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace arrowhip {
namespace like {

constexpr uint8_t kAnchorStart = 1, kAnchorEnd = 2;

inline std::vector<uint8_t> Emit(const std::vector<std::vector<uint8_t>>& segments, uint8_t flags) {
  std::vector<uint8_t> prog;
  prog.push_back(segments.empty() ? (uint8_t)0 : flags);
  prog.push_back((uint8_t)(segments.size() & 0xFF));
  prog.push_back((uint8_t)(segments.size() >> 8));
  for (const auto& s : segments) {
    const size_t ne = s.size() / 2;
    prog.push_back((uint8_t)(ne & 0xFF));
    prog.push_back((uint8_t)(ne >> 8));
    prog.insert(prog.end(), s.begin(), s.end());
  }
  return prog;
}

inline std::vector<uint8_t> Compile(const uint8_t* pattern, size_t n) {
  // Arrow's three shortcuts: the runs of `%` at both ends, and what stands between them taken raw
  size_t a = 0, b = n;
  while (a < n && pattern[a] == '%') a++;
  while (b > a && pattern[b - 1] == '%') b--;
  const bool lead = a > 0, trail = b < n;
  bool wild = false;
  for (size_t i = a; i < b; i++) wild = wild || pattern[i] == '%' || pattern[i] == '_';
  if (a == b && lead) return Emit({}, 0);   // only `%`: every row
  if (!wild && a < b && (lead || trail) && (pattern[b - 1] != '\\' || !trail)) {
    std::vector<uint8_t> lit;
    for (size_t i = a; i < b; i++) {
      lit.push_back(0);
      lit.push_back(pattern[i]);
    }
    return Emit({lit}, (uint8_t)((lead ? 0 : kAnchorStart) | (trail ? 0 : kAnchorEnd)));
  }
  // every other pattern: escapes resolved, segments cut at the unescaped `%`
  std::vector<std::vector<uint8_t>> segments;
  std::vector<uint8_t> cur;
  bool starts_with_percent = false, ends_with_percent = false;
  auto close = [&]() {
    if (!cur.empty()) segments.push_back(cur);
    cur.clear();
  };
  for (size_t i = 0; i < n; i++) {
    const uint8_t c = pattern[i];
    if (c == '%') {
      if (i == 0) starts_with_percent = true;
      close();
      ends_with_percent = true;
      continue;
    }
    if (c == '\\') {
      if (i + 1 == n) break;   // a lone escape character at the end is dropped
      ends_with_percent = false;
      cur.push_back(0);
      cur.push_back(pattern[++i]);
      continue;
    }
    ends_with_percent = false;
    cur.push_back(c == '_' ? 1 : 0);
    cur.push_back(c == '_' ? 0 : c);
  }
  close();
  if (segments.empty() && !starts_with_percent) segments.emplace_back();   // no `%`, no character: the row must be empty
  return Emit(segments, (uint8_t)((starts_with_percent ? 0 : kAnchorStart) | (ends_with_percent ? 0 : kAnchorEnd)));
}

}  // namespace like
}  // namespace arrowhip
