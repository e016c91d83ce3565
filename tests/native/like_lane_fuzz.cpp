// Stand-alone fuzz of delta_amd/csrc/like_lane.h for a sanitizer build (tests/test_like_lane.py builds
// it with -fsanitize=address,undefined and runs it): random patterns and values, every value in a heap
// block of exactly its length so a read past it is caught, the results compared with a plain
// restatement of the character definition (a dynamic program over characters).
#include "../../delta_amd/csrc/like_lane.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

using namespace dr::lk;
typedef std::vector<std::string> Chars;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return uint32_t((rng_state >> 11) % n);
}

// one non-continuation byte plus the continuation bytes after it; leading continuation bytes alone
static Chars split(const std::string& s) {
  Chars out;
  for (size_t k = 0; k < s.size(); ++k) {
    if (is_cont(uint8_t(s[k])) && !out.empty() && !is_cont(uint8_t(out.back()[0]))) out.back().push_back(s[k]);
    else out.emplace_back(1, s[k]);
  }
  return out;
}

struct PTok { int kind; std::string ch; };  // 0 a character, 1 `_`, 2 `%`
static bool parse(const std::string& pat, const std::string& esc, std::vector<PTok>* out) {
  const Chars c = split(pat);
  for (size_t k = 0; k < c.size(); ++k) {
    if (c[k] == esc) {
      if (k + 1 == c.size() || (c[k + 1] != "_" && c[k + 1] != "%" && c[k + 1] != esc)) return false;
      out->push_back(PTok{0, c[++k]});
    } else if (c[k] == "_") out->push_back(PTok{1, ""});
    else if (c[k] == "%") out->push_back(PTok{2, ""});
    else out->push_back(PTok{0, c[k]});
  }
  return true;
}
static bool ref_match(const Chars& v, const std::vector<PTok>& p) {
  std::vector<char> cur(v.size() + 1, 0), nxt;
  cur[0] = 1;
  for (const PTok& t : p) {
    nxt.assign(v.size() + 1, 0);
    if (t.kind == 2) {
      bool on = false;
      for (size_t k = 0; k <= v.size(); ++k) { on = on || cur[k]; nxt[k] = on; }
    } else {
      for (size_t k = 0; k < v.size(); ++k)
        if (cur[k] && (t.kind == 1 || v[k] == t.ch)) nxt[k + 1] = 1;
    }
    cur.swap(nxt);
  }
  return cur[v.size()] != 0;
}

static const char* kAlphabet[] = {"a", "b", "c", "d", "%", "_", "\\", "\xC3\xA9", "\n", "\xE2\x82\xAC", "\xF0\x9F\x98\x80"};

static std::string random_text(bool raw, uint32_t maxlen, bool wild) {
  std::string s;
  const uint32_t n = rnd(maxlen + 1);
  for (uint32_t k = 0; k < n; ++k) {
    if (raw) s.push_back(char(rnd(4) ? (rnd(2) ? 0x80 + rnd(64) : 'a' + rnd(3)) : rnd(256)));
    else s += kAlphabet[wild ? rnd(11) : (rnd(8) < 7 ? rnd(4) : 4 + rnd(7))];
  }
  return s;
}

static int check(const std::string& value, const std::string& pat, uint32_t escape, const std::string& esc) {
  std::unique_ptr<uint8_t[]> v(new uint8_t[value.size()]), p(new uint8_t[pat.size()]);
  std::memcpy(v.get(), value.data(), value.size());
  std::memcpy(p.get(), pat.data(), pat.size());
  const LikeCompiled c = like_compile(p.get(), pat.size(), escape);
  std::vector<PTok> toks;
  const bool valid = parse(pat, esc, &toks);
  if (valid != c.error.empty()) {
    std::fprintf(stderr, "validity differs: pattern '%s' (%s)\n", pat.c_str(), c.error.c_str());
    return 1;
  }
  if (!valid) return 0;
  std::unique_ptr<uint8_t[]> t(new uint8_t[c.text.size()]);
  std::memcpy(t.get(), c.text.data(), c.text.size());
  const uint32_t n = uint32_t(value.size()), tn = uint32_t(c.text.size());
  bool got;
  switch (c.kind) {
    case LIKE_EQ: got = n == tn && bytes_eq(v.get(), t.get(), n); break;
    case LIKE_STARTSWITH: got = starts_with(v.get(), n, t.get(), tn); break;
    case LIKE_ENDSWITH: got = ends_with(v.get(), n, t.get(), tn); break;
    case LIKE_CONTAINS: got = contains(v.get(), n, t.get(), tn); break;
    default: got = like_match(v.get(), n, t.get(), tn);
  }
  // the folded tests are bytewise: they agree with the character definition when the value's
  // characters are whole where the needle ends and begins, which valid UTF-8 guarantees
  const bool want = ref_match(split(value), toks);
  if (got != want) {
    std::fprintf(stderr, "mismatch: value (%u bytes) pattern '%s' kind %d: got %d want %d\n", n, pat.c_str(), c.kind, int(got), int(want));
    for (uint32_t k = 0; k < n; ++k) std::fprintf(stderr, " %02x", v[k]);
    std::fprintf(stderr, "\n");
    return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  const uint32_t rounds = argc > 1 ? uint32_t(std::atoi(argv[1])) : 200000;
  uint32_t bad = 0;
  for (uint32_t r = 0; r < rounds && !bad; ++r) {
    // valid UTF-8 on both sides: the folded shapes and the programs
    bad += check(random_text(false, 12, false), random_text(false, 8, true), '\\', "\\");
    // any bytes in the value; the pattern keeps at least one `_` between its `%`s often enough that
    // most compile to programs (the folded bytewise tests are Spark's own on any bytes, but do not
    // follow the character definition on malformed values, so only programs are compared there)
    const std::string pat = random_text(false, 8, true);
    const LikeCompiled c = like_compile(reinterpret_cast<const uint8_t*>(pat.data()), pat.size(), '#');
    const std::string value = random_text(true, 12, false);
    if (c.error.empty() && c.kind != LIKE_PROGRAM) {  // still run for the sanitizer, result not compared
      std::unique_ptr<uint8_t[]> v(new uint8_t[value.size()]);
      std::memcpy(v.get(), value.data(), value.size());
      const uint8_t* t = reinterpret_cast<const uint8_t*>(c.text.data());
      (void)starts_with(v.get(), uint32_t(value.size()), t, uint32_t(c.text.size()));
      (void)ends_with(v.get(), uint32_t(value.size()), t, uint32_t(c.text.size()));
      (void)contains(v.get(), uint32_t(value.size()), t, uint32_t(c.text.size()));
    } else {
      bad += check(value, pat, '#', "#");
    }
    // a multi-byte escape character
    bad += check(random_text(false, 10, false), random_text(false, 8, true), 0xE9, "\xC3\xA9");
  }
  if (bad) return 1;
  std::printf("like_lane fuzz ok: %u rounds\n", rounds);
  return 0;
}
