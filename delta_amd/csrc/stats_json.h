// K5 data skipping: where the wanted statistics sit in one `add.stats` string (PROTOCOL.md, "Per-file
// Statistics": {"numRecords":n,"minValues":{..},"maxValues":{..},"nullCount":{..}}, struct columns
// nested). One source for k_stats_extract (k_filter.hip) and for the host
// (tests/native/stats_json_host.cpp): no HIP type, g++ compiles it alone.
//
// locate() makes one forward pass over the string -- no recursion, no allocation, every read bounded
// by n -- and answers, for up to PV_MAXC wanted (source, path) pairs, the token of each: where it
// starts, how long it is and what kind it is. The pass is a strict JSON reader (RFC 8259: the four
// whitespace bytes, no control byte in a string, the eight escapes and \uXXXX, numbers as
// -?(0|[1-9][0-9]*)(.[0-9]+)?([eE][+-]?[0-9]+)?, the three literals, nothing but whitespace after the
// value), because Spark's from_json yields NULL for a record its parser refuses (PERMISSIVE mode), and
// NULL statistics keep the file: a string it refuses -- truncated, a bad token anywhere, nesting beyond
// SJ_MAXDEPTH -- or whose value is no object gives SJ_ABSENT for every pair, never an error.
// Values that are not wanted are walked by the same reader, so `"}{"` inside a string is no structure
// and `\"` ends no string. A key is compared with its escapes resolved (`a` then the \u escape of 0062 is the key ab); a
// repeated key keeps the last value at every level, as Jackson and Spark's struct conversion
// overwrite; a path segment whose value is no object gives SJ_ABSENT below it.
#pragma once
#include <cstdint>

#include "filter_plan.h"

namespace dr {
namespace sj {

// dr_pred column sources (include/deltareplay.h DR_SRC_*)
enum : int32_t { SRC_PARTITION = 0, SRC_MIN = 1, SRC_MAX = 2, SRC_NULLCOUNT = 3, SRC_NUMRECORDS = 4 };
enum Kind : uint8_t {
  SJ_ABSENT = 0,          // no such member (or a malformed string)
  SJ_NULL = 1,            // the JSON literal null
  SJ_NUMBER = 2,          // [ptr, ptr + len): the number's text
  SJ_STRING_RAW = 3,      // [ptr, ptr + len): the bytes between the quotes, no escape among them
  SJ_STRING_ESCAPED = 4,  // the same, holding escapes
  SJ_OTHER = 5            // an object, an array, true or false: ptr at its first byte, len 0
};
constexpr int SJ_MAXSEG = 8;      // segments of a path
constexpr int SJ_MAXPATH = 255;   // bytes of a path, separators included
constexpr int SJ_MAXDEPTH = 64;   // open containers (one bit each)
constexpr uint8_t SJ_SEP = 0x01;  // joins the segments of a nested struct leaf's path

struct Want {
  int32_t source;       // SRC_MIN .. SRC_NUMRECORDS
  const uint8_t* path;  // the data column's field names, exactly as the JSON keys, joined by SJ_SEP
  uint32_t path_len;    // 0 for SRC_NUMRECORDS
};
struct Found {
  const uint8_t* ptr;
  uint32_t len;
  uint8_t kind;
};

DR_HD inline bool sj_ws(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
DR_HD inline int sj_hex(uint8_t c) {
  return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
}

// The string whose opening quote is at s[i - 1]: the index of its closing quote, or n when it is
// truncated or malformed. *esc: it holds a backslash.
DR_HD inline uint64_t sj_string_end(const uint8_t* s, uint64_t n, uint64_t i, bool* esc) {
  *esc = false;
  while (i < n) {
    const uint8_t c = s[i];
    if (c == '"') return i;
    if (c < 0x20) return n;
    if (c != '\\') { ++i; continue; }
    *esc = true;
    if (i + 1 >= n) return n;
    const uint8_t e = s[i + 1];
    if (e == 'u') {
      if (i + 6 > n) return n;
      for (int k = 2; k < 6; ++k)
        if (sj_hex(s[i + k]) < 0) return n;
      i += 6;
    } else if (e == '"' || e == '\\' || e == '/' || e == 'b' || e == 'f' || e == 'n' || e == 'r' || e == 't') {
      i += 2;
    } else {
      return n;
    }
  }
  return n;
}

// The number starting at s[i]: the index after it, or n + 1 when it is no number.
DR_HD inline uint64_t sj_number_end(const uint8_t* s, uint64_t n, uint64_t i) {
  auto digit = [&](uint64_t k) { return k < n && s[k] >= '0' && s[k] <= '9'; };
  if (i < n && s[i] == '-') ++i;
  if (!digit(i)) return n + 1;
  if (s[i] == '0') ++i;
  else while (digit(i)) ++i;
  if (i < n && s[i] == '.') {
    if (!digit(i + 1)) return n + 1;
    ++i;
    while (digit(i)) ++i;
  }
  if (i < n && (s[i] == 'e' || s[i] == 'E')) {
    uint64_t k = i + 1;
    if (k < n && (s[k] == '+' || s[k] == '-')) ++k;
    if (!digit(k)) return n + 1;
    while (digit(k)) ++k;
    i = k;
  }
  return i;
}

// The well-formed JSON string body k[0 .. kn) (escapes included when esc), resolved, == t[0 .. tn)?
// \uXXXX becomes UTF-8, a surrogate pair one code point, a lone surrogate its three bytes.
DR_HD inline bool sj_key_eq(const uint8_t* k, uint32_t kn, bool esc, const uint8_t* t, uint32_t tn) {
  if (!esc) {
    if (kn != tn) return false;
    for (uint32_t q = 0; q < kn; ++q)
      if (k[q] != t[q]) return false;
    return true;
  }
  uint32_t o = 0;
  bool same = true;  // every resolved byte so far equals the target's
  auto put = [&](uint32_t b) {
    same = same && o < tn && t[o] == uint8_t(b);
    ++o;
  };
  for (uint32_t i = 0; i < kn;) {
    uint8_t c = k[i++];
    if (c != '\\') {
      put(c);
      continue;
    }
    c = k[i++];
    if (c != 'u') {
      const uint8_t v = c == 'b' ? '\b' : c == 'f' ? '\f' : c == 'n' ? '\n' : c == 'r' ? '\r' : c == 't' ? '\t' : c;
      put(v);
      continue;
    }
    uint32_t cp = 0;
    for (int q = 0; q < 4; ++q) cp = cp * 16 + uint32_t(sj_hex(k[i++]));
    if (cp >= 0xD800 && cp < 0xDC00 && i + 6 <= kn && k[i] == '\\' && k[i + 1] == 'u') {
      uint32_t lo = 0;
      for (int q = 0; q < 4; ++q) lo = lo * 16 + uint32_t(sj_hex(k[i + 2 + q]));
      if (lo >= 0xDC00 && lo < 0xE000) {
        cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
        i += 6;
      }
    }
    if (cp < 0x80) {
      put(cp);
    } else if (cp < 0x800) {
      put(0xC0 | (cp >> 6));
      put(0x80 | (cp & 63));
    } else if (cp < 0x10000) {
      put(0xE0 | (cp >> 12));
      put(0x80 | ((cp >> 6) & 63));
      put(0x80 | (cp & 63));
    } else {
      put(0xF0 | (cp >> 18));
      put(0x80 | ((cp >> 12) & 63));
      put(0x80 | ((cp >> 6) & 63));
      put(0x80 | (cp & 63));
    }
    if (!same) return false;
  }
  return same && o == tn;
}

// Component q of a want -- 0: the member of the statistics object its source names, 1 ..: the path's
// segments -- as bytes; false when the want has no such component.
DR_HD inline bool sj_component(const Want& w, int q, const uint8_t** b, uint32_t* len) {
  if (q == 0) {
    const char* name = w.source == SRC_MIN ? "minValues" : w.source == SRC_MAX ? "maxValues"
                     : w.source == SRC_NULLCOUNT ? "nullCount" : "numRecords";
    *b = reinterpret_cast<const uint8_t*>(name);
    *len = w.source == SRC_NUMRECORDS ? 10 : 9;
    return true;
  }
  if (w.source == SRC_NUMRECORDS) return false;
  uint32_t at = 0;
  for (int seg = 1; seg < q; ++seg) {
    while (at < w.path_len && w.path[at] != SJ_SEP) ++at;
    if (at >= w.path_len) return false;
    ++at;
  }
  uint32_t e = at;
  while (e < w.path_len && w.path[e] != SJ_SEP) ++e;
  *b = w.path + at;
  *len = e - at;
  return true;
}
DR_HD inline int sj_components(const Want& w) {
  if (w.source == SRC_NUMRECORDS) return 1;
  int c = 2;
  for (uint32_t q = 0; q < w.path_len; ++q) c += w.path[q] == SJ_SEP;
  return c;
}

DR_HD inline void locate(const uint8_t* s, uint64_t n, const Want* want, int nwant, Found* out) {
  if (nwant > PV_MAXC) nwant = PV_MAXC;
  // matched[w]: how many components of want w the chain of open objects has matched; it is compared
  // further only while that chain is all there is (depth == tracked)
  uint8_t matched[PV_MAXC], ncomp[PV_MAXC];
  for (int w = 0; w < nwant; ++w) {
    out[w] = Found{nullptr, 0, SJ_ABSENT};
    matched[w] = 0;
    ncomp[w] = uint8_t(sj_components(want[w]));
  }
  auto fail = [&]() {
    for (int w = 0; w < nwant; ++w) out[w] = Found{nullptr, 0, SJ_ABSENT};
  };
  uint64_t i = 0;
  while (i < n && sj_ws(s[i])) ++i;
  if (i >= n || s[i] != '{') return;  // no object (whatever else it is): nothing is there
  uint64_t kinds = 1;  // one bit per open container, the innermost lowest: 1 an object, 0 an array
  int depth = 1, tracked = 1;
  ++i;
  // what the reader expects next
  enum { FIRST_KEY, KEY, FIRST_ELEM, VALUE, AFTER_VALUE } st = FIRST_KEY;
  uint32_t hit = 0;  // wants whose next component the last key matched (bit w), for the value after it
  while (depth > 0) {
    while (i < n && sj_ws(s[i])) ++i;
    if (i >= n) return fail();
    const uint8_t c = s[i];
    if (st == FIRST_KEY || st == KEY) {
      if (c == '}' && st == FIRST_KEY) {
        st = AFTER_VALUE;  // falls into the close below
      } else {
        if (c != '"') return fail();
        bool esc;
        const uint64_t q = sj_string_end(s, n, i + 1, &esc);
        if (q >= n) return fail();
        hit = 0;
        if (depth == tracked)
          for (int w = 0; w < nwant; ++w) {
            const uint8_t* b;
            uint32_t len;
            if (matched[w] == depth - 1 && matched[w] < ncomp[w] && sj_component(want[w], depth - 1, &b, &len) &&
                sj_key_eq(s + i + 1, uint32_t(q - i - 1), esc, b, len))
              hit |= 1u << w;
          }
        i = q + 1;
        while (i < n && sj_ws(s[i])) ++i;
        if (i >= n || s[i] != ':') return fail();
        ++i;
        st = VALUE;
        continue;
      }
    }
    if (st == FIRST_ELEM && c == ']') st = AFTER_VALUE;
    if (st == AFTER_VALUE) {
      if (c == ',') {
        st = (kinds & 1) ? KEY : VALUE;
        ++i;
        continue;
      }
      if (c != ((kinds & 1) ? '}' : ']')) return fail();
      if (depth == tracked) {
        for (int w = 0; w < nwant; ++w)
          if (matched[w] == depth - 1 && depth >= 2) matched[w] = uint8_t(depth - 2);
        --tracked;
      }
      kinds >>= 1;
      --depth;
      ++i;
      continue;
    }
    // a value (VALUE, or the first element of an array)
    Found f{s + i, 0, SJ_OTHER};
    bool opens = false;
    if (c == '"') {
      bool esc;
      const uint64_t q = sj_string_end(s, n, i + 1, &esc);
      if (q >= n) return fail();
      f = Found{s + i + 1, uint32_t(q - i - 1), uint8_t(esc ? SJ_STRING_ESCAPED : SJ_STRING_RAW)};
      i = q + 1;
    } else if (c == '{' || c == '[') {
      opens = true;
    } else if (c == '-' || (c >= '0' && c <= '9')) {
      const uint64_t q = sj_number_end(s, n, i);
      if (q > n) return fail();
      f = Found{s + i, uint32_t(q - i), SJ_NUMBER};
      i = q;
    } else {
      const char* word = c == 'n' ? "null" : c == 't' ? "true" : c == 'f' ? "false" : nullptr;
      if (!word) return fail();
      uint64_t q = 0;
      for (; word[q]; ++q)
        if (i + q >= n || s[i + q] != uint8_t(word[q])) return fail();
      if (c == 'n') f.kind = SJ_NULL;
      i += q;
    }
    bool descend = false;
    for (int w = 0; w < nwant && hit; ++w) {
      if (!(hit >> w & 1)) continue;
      if (depth == ncomp[w]) {
        out[w] = f;  // the last of a repeated key
      } else {
        out[w] = Found{nullptr, 0, SJ_ABSENT};  // a repeated member replaces the earlier one whole
        if (opens && c == '{') {
          matched[w] = uint8_t(depth);
          descend = true;
        }
      }
    }
    hit = 0;
    if (opens) {
      if (depth >= SJ_MAXDEPTH) return fail();
      if (descend) tracked = depth + 1;
      kinds = (kinds << 1) | (c == '{' ? 1u : 0u);
      ++depth;
      ++i;
      st = c == '{' ? FIRST_KEY : FIRST_ELEM;
      continue;
    }
    st = AFTER_VALUE;
  }
  while (i < n && sj_ws(s[i])) ++i;
  if (i != n) fail();  // something after the object
}

}  // namespace sj
}  // namespace dr
