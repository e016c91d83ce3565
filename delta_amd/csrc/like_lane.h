// K5 string pattern predicates: Catalyst's StartsWith / EndsWith / Contains (UTF8String's bytewise
// prefix, suffix and substring tests) and Like (StringUtils.escapeLikeRegex, then a full match with
// (?s): `_` is exactly one code point, newline included, `%` any run, everything else itself).
//
// LIKE is compiled once per call on the host (like_compile) into a byte program the lanes interpret
// (like_match). The pattern is cut at its `%`s into segments; a segment is a sequence of tokens,
// each a literal byte run or "k characters of any kind", so a segment has a fixed length in
// characters. Matching is greedy: the first segment at the start when the pattern does not begin with
// `%`, the last segment backwards from the end when it does not end with `%`, every other segment at
// the leftmost position after the one before it. That is exact for fixed-length segments, costs
// O(n * m) and needs neither backtracking across segments, recursion nor a local array.
//
//   prog[0]     flags: LK_HEAD the pattern does not begin with `%`, LK_TAIL it does not end with `%`
//   prog[1]     0
//   prog[2..3]  number of segments (little-endian; empty segments are dropped: `a%%b` has two)
//   a segment:  u16 byte length of its tokens, then the tokens
//   a token:    LK_LIT  len byte*len   a run of 1..255 literal bytes (whole UTF-8 characters)
//               LK_ANY  k              1..255 characters of any kind
// The tokens of the last segment of a LK_TAIL pattern that has a `%` are stored last-first: it is
// matched backwards from the end of the value (with a `_` in it, its length in bytes varies).
//
// A character of a value is one non-continuation byte and the continuation bytes (10xxxxxx) after it;
// continuation bytes before the first other byte are one character each. For valid UTF-8 that is a
// code point. Java decodes malformed values with replacement characters first; this definition
// stands in for that (parity unpinned). Every read of the value is bounded by its length.
//
// Written for HIP device code and for the host (tests/native/like_lane_host.cpp builds it with g++ to
// fuzz it against Python's re module).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define LK_HD __host__ __device__ __forceinline__
#else
#define LK_HD inline
#endif

namespace dr {
namespace lk {

enum : uint8_t { LK_HEAD = 1, LK_TAIL = 2 };
enum : uint8_t { LK_LIT = 0, LK_ANY = 1 };

LK_HD bool is_cont(uint8_t b) { return (b & 0xC0u) == 0x80u; }

LK_HD bool bytes_eq(const uint8_t* a, const uint8_t* b, uint32_t n) {
  for (uint32_t k = 0; k < n; ++k)
    if (a[k] != b[k]) return false;
  return true;
}

// ---- UTF8String.startsWith / endsWith / contains ----------------------------------------------------
LK_HD bool starts_with(const uint8_t* s, uint32_t n, const uint8_t* p, uint32_t m) {
  return m <= n && bytes_eq(s, p, m);
}
LK_HD bool ends_with(const uint8_t* s, uint32_t n, const uint8_t* p, uint32_t m) {
  return m <= n && bytes_eq(s + (n - m), p, m);
}
LK_HD bool contains(const uint8_t* s, uint32_t n, const uint8_t* p, uint32_t m) {
  if (m > n) return false;
  for (uint32_t at = 0; at + m <= n; ++at)
    if (bytes_eq(s + at, p, m)) return true;
  return false;
}

// ---- LIKE -----------------------------------------------------------------------------------------
constexpr uint32_t LK_FAIL = 0xffffffffu;

// One segment (tokens t[0, tn)) forwards from the character boundary `at`, within s[0, lim): the
// position after it, or LK_FAIL. A literal run must end on a character boundary of the value.
LK_HD uint32_t seg_fwd(const uint8_t* s, uint32_t n, uint32_t lim, uint32_t at, const uint8_t* t, uint32_t tn) {
  uint32_t q = 0;
  while (q + 2 <= tn) {
    const uint32_t kind = t[q], len = t[q + 1];
    q += 2;
    if (kind == LK_LIT) {
      if (q + len > tn || len > lim - at || !bytes_eq(s + at, t + q, len)) return LK_FAIL;
      at += len;
      q += len;
      if (at < n && is_cont(s[at])) return LK_FAIL;
    } else {
      for (uint32_t k = 0; k < len; ++k) {
        if (at >= lim) return LK_FAIL;
        const bool lead = !is_cont(s[at]);
        ++at;
        while (lead && at < n && is_cont(s[at])) ++at;
      }
      if (at > lim) return LK_FAIL;
    }
  }
  return at;
}

// One segment whose tokens are stored last-first, backwards from the character boundary `end`: the
// position it starts at, or LK_FAIL.
LK_HD uint32_t seg_bwd(const uint8_t* s, uint32_t end, const uint8_t* t, uint32_t tn) {
  uint32_t q = 0;
  while (q + 2 <= tn) {
    const uint32_t kind = t[q], len = t[q + 1];
    q += 2;
    if (kind == LK_LIT) {
      if (q + len > tn || len > end || !bytes_eq(s + (end - len), t + q, len)) return LK_FAIL;
      end -= len;
      q += len;
    } else {
      for (uint32_t k = 0; k < len; ++k) {
        if (end == 0) return LK_FAIL;
        uint32_t b = end - 1;
        while (b > 0 && is_cont(s[b])) --b;
        end = is_cont(s[b]) ? end - 1 : b;  // nothing but continuation bytes before it: one byte
      }
    }
  }
  return end;
}

// The value s[0, n) against the compiled pattern prog[0, plen).
LK_HD bool like_match(const uint8_t* s, uint32_t n, const uint8_t* prog, uint32_t plen) {
  if (plen < 4) return false;
  const uint32_t flags = prog[0];
  uint32_t nseg = uint32_t(prog[2]) | (uint32_t(prog[3]) << 8);
  if (nseg == 0) return (flags & LK_HEAD) ? n == 0 : true;
  const bool whole = flags == (LK_HEAD | LK_TAIL) && nseg == 1;  // no `%` at all
  uint32_t q = 4, pos = 0, lim = n;
  if ((flags & LK_TAIL) && !whole) {
    // the last segment, from the end; then the others must fit in front of it
    uint32_t z = 4;
    for (uint32_t k = 0; k + 1 < nseg; ++k) {
      if (z + 2 > plen) return false;
      z += 2 + (uint32_t(prog[z]) | (uint32_t(prog[z + 1]) << 8));
    }
    if (z + 2 > plen) return false;
    const uint32_t tn = uint32_t(prog[z]) | (uint32_t(prog[z + 1]) << 8);
    if (z + 2 + tn > plen) return false;
    lim = seg_bwd(s, n, prog + z + 2, tn);
    if (lim == LK_FAIL) return false;
    --nseg;
  }
  for (uint32_t k = 0; k < nseg; ++k) {
    if (q + 2 > plen) return false;
    const uint32_t tn = uint32_t(prog[q]) | (uint32_t(prog[q + 1]) << 8);
    const uint8_t* t = prog + q + 2;
    q += 2 + tn;
    if (q > plen || tn < 2) return false;
    if (k == 0 && (flags & LK_HEAD)) {
      pos = seg_fwd(s, n, lim, 0, t, tn);
      if (pos == LK_FAIL) return false;
      if (whole) return pos == n;
      continue;
    }
    // leftmost. A segment that begins with a literal can only match at a character boundary (its
    // first byte is no continuation byte); one that begins with `_` is tried at boundaries only: at
    // a non-continuation byte, and inside the continuation bytes the value may begin with (run).
    const bool any_first = t[0] == LK_ANY;
    bool run = true;
    for (uint32_t b = 0; any_first && run && b < pos; ++b) run = is_cont(s[b]);
    uint32_t e = LK_FAIL;
    for (uint32_t at = pos; at < lim; ++at) {
      const bool cont = is_cont(s[at]);
      if (any_first && at > pos && cont && !run) continue;
      run = run && cont;
      e = seg_fwd(s, n, lim, at, t, tn);
      if (e != LK_FAIL) break;
    }
    if (e == LK_FAIL) return false;
    pos = e;
  }
  return true;
}

// ---- host: the pattern compiler ----------------------------------------------------------------------
// What a pattern compiles to: the simple shapes fold into the cheaper tests (`text` holds the needle),
// the rest into a LIKE program (`text` holds the program).
enum LikeKind : int { LIKE_EQ = 0, LIKE_STARTSWITH = 1, LIKE_ENDSWITH = 2, LIKE_CONTAINS = 3, LIKE_PROGRAM = 4 };
struct LikeCompiled {
  int kind = LIKE_PROGRAM;
  std::string text;
  std::string error;  // not empty: the pattern is invalid (Spark's message)
};

// Decodes one UTF-8 code point of p[at, n) (strict: no overlong forms, surrogates or values past
// U+10FFFF); returns its length, 0 if malformed.
inline uint32_t utf8_decode(const uint8_t* p, size_t at, size_t n, uint32_t* cp) {
  const uint8_t b = p[at];
  uint32_t len, v, lo;
  if (b < 0x80) { *cp = b; return 1; }
  if ((b & 0xE0) == 0xC0) { len = 2; v = b & 0x1Fu; lo = 0x80; }
  else if ((b & 0xF0) == 0xE0) { len = 3; v = b & 0x0Fu; lo = 0x800; }
  else if ((b & 0xF8) == 0xF0) { len = 4; v = b & 0x07u; lo = 0x10000; }
  else return 0;
  if (at + len > n) return 0;
  for (uint32_t k = 1; k < len; ++k) {
    if (!is_cont(p[at + k])) return 0;
    v = (v << 6) | (p[at + k] & 0x3Fu);
  }
  if (v < lo || v > 0x10FFFF || (v >= 0xD800 && v <= 0xDFFF)) return 0;
  *cp = v;
  return len;
}

inline std::string utf8_text(const uint8_t* p, uint32_t len) { return std::string(reinterpret_cast<const char*>(p), len); }

// StringUtils.escapeLikeRegex, read code point by code point: the escape character before `_`, `%`
// or itself gives that character; before anything else, or last, it is an error; the escape test comes
// before the wildcard test.
inline LikeCompiled like_compile(const uint8_t* pat, size_t n, uint32_t escape) {
  LikeCompiled out;
  if (escape < 1 || escape > 0xFFFF || (escape >= 0xD800 && escape <= 0xDFFF)) {
    out.error = "the escape character must be one character (a code point in 1..0xFFFF, no surrogate)";
    return out;
  }
  struct Tok { int kind; std::string lit; uint32_t any; };  // kind: 0 literal, 1 any, 2 `%`
  std::vector<Tok> toks;
  auto lit = [&](const uint8_t* p, uint32_t len) {
    if (toks.empty() || toks.back().kind != 0) toks.push_back(Tok{0, std::string(), 0});
    toks.back().lit += utf8_text(p, len);
  };
  size_t at = 0;
  while (at < n) {
    uint32_t cp = 0;
    const uint32_t len = utf8_decode(pat, at, n, &cp);
    if (!len) {
      out.error = "the pattern is not valid UTF-8";
      return out;
    }
    if (cp == escape) {
      if (at + len >= n) {
        out.error = "the pattern '" + utf8_text(pat, uint32_t(n)) + "' is invalid, it is not allowed to end with the escape character";
        return out;
      }
      uint32_t c2 = 0;
      const uint32_t len2 = utf8_decode(pat, at + len, n, &c2);
      if (!len2) {
        out.error = "the pattern is not valid UTF-8";
        return out;
      }
      if (c2 != '_' && c2 != '%' && c2 != escape) {
        out.error = "the pattern '" + utf8_text(pat, uint32_t(n)) + "' is invalid, the escape character is not allowed to precede '" +
                    utf8_text(pat + at + len, len2) + "'";
        return out;
      }
      lit(pat + at + len, len2);
      at += len + len2;
      continue;
    }
    if (cp == '_') {
      if (toks.empty() || toks.back().kind != 1) toks.push_back(Tok{1, std::string(), 0});
      ++toks.back().any;
    } else if (cp == '%') {
      if (toks.empty() || toks.back().kind != 2) toks.push_back(Tok{2, std::string(), 0});
    } else {
      lit(pat + at, len);
    }
    at += len;
  }
  // the simple shapes
  const size_t nt = toks.size();
  auto is = [&](size_t k, int kind) { return k < nt && toks[k].kind == kind; };
  if (nt == 0) { out.kind = LIKE_EQ; return out; }
  if (nt == 1 && is(0, 0)) { out.kind = LIKE_EQ; out.text = toks[0].lit; return out; }
  if (nt == 1 && is(0, 2)) { out.kind = LIKE_STARTSWITH; return out; }  // `%`: every non-NULL value
  if (nt == 2 && is(0, 0) && is(1, 2)) { out.kind = LIKE_STARTSWITH; out.text = toks[0].lit; return out; }
  if (nt == 2 && is(0, 2) && is(1, 0)) { out.kind = LIKE_ENDSWITH; out.text = toks[1].lit; return out; }
  if (nt == 3 && is(0, 2) && is(1, 0) && is(2, 2)) { out.kind = LIKE_CONTAINS; out.text = toks[1].lit; return out; }
  // the program
  const bool head = toks.front().kind != 2, tail = toks.back().kind != 2;
  std::vector<std::vector<Tok>> segs;
  bool open = false, any_pct = false;
  for (const Tok& t : toks) {
    if (t.kind == 2) { open = false; any_pct = true; continue; }
    if (!open) { segs.emplace_back(); open = true; }
    segs.back().push_back(t);
  }
  if (segs.size() > 0xFFFF) {
    out.error = "the pattern has too many segments";
    return out;
  }
  std::string prog;
  prog.push_back(char((head ? LK_HEAD : 0) | (tail ? LK_TAIL : 0)));
  prog.push_back(0);
  prog.push_back(char(segs.size() & 0xFF));
  prog.push_back(char(segs.size() >> 8));
  for (size_t k = 0; k < segs.size(); ++k) {
    // runs longer than 255 are cut (a literal run between characters)
    std::vector<std::string> enc;
    for (const Tok& t : segs[k]) {
      if (t.kind == 1) {
        for (uint32_t left = t.any; left;) {
          const uint32_t c = left < 255 ? left : 255;
          enc.push_back(std::string{char(LK_ANY), char(c)});
          left -= c;
        }
        continue;
      }
      size_t b = 0;
      while (b < t.lit.size()) {
        size_t e = t.lit.size() - b <= 255 ? t.lit.size() : b + 255;
        while (e < t.lit.size() && is_cont(uint8_t(t.lit[e]))) --e;
        enc.push_back(std::string{char(LK_LIT), char(e - b)} + t.lit.substr(b, e - b));
        b = e;
      }
    }
    if (tail && any_pct && k + 1 == segs.size()) enc = std::vector<std::string>(enc.rbegin(), enc.rend());
    std::string body;
    for (const std::string& x : enc) body += x;
    if (body.size() > 0xFFFF) {
      out.error = "the pattern is too long";
      return out;
    }
    prog.push_back(char(body.size() & 0xFF));
    prog.push_back(char(body.size() >> 8));
    prog += body;
  }
  out.kind = LIKE_PROGRAM;
  out.text = prog;
  return out;
}

}  // namespace lk
}  // namespace dr
