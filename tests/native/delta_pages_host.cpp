// Prints leaves of a Parquet file as the host decoder (parquet_meta.cpp) reads them, for
// tests/test_delta_pages_host.py: every row group's levels and values through decode_column_host, then
// the same leaf through sparse_entries (threshold 0), which must agree.
//   delta_pages_host FILE LEAF...
// Output per leaf: "leaf NAME", "levels N", then one line per level "<def> <rep> <value>" (integers in
// decimal, byte arrays in hex with an 'x' in front, '-' for no value), then "ok". A dr::Error prints
// "DR_E_PARQUET: text" (or "DR_E_<n>: text" for another status) to stderr and exits 3.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../delta_amd/csrc/common.h"
#include "../../delta_amd/csrc/parquet_meta.h"

using namespace dr::pq;

static void print_leaf(const std::vector<uint8_t>& file, const FileMeta& meta, const std::string& leaf_name) {
  const Leaf* leaf = meta.leaf(leaf_name);
  if (!leaf) dr::fail(DR_E_INVALID_ARG, "no leaf " + leaf_name);
  std::string out;
  size_t levels = 0;
  int64_t row_base = 0;
  auto put = [&](int def, int rep, bool has, int64_t iv, const std::string& sv) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%d %d ", def, rep);
    out += buf;
    if (!has) {
      out += "-";
    } else if (leaf->type == BYTE_ARRAY) {
      out += "x";
      for (unsigned char c : sv) {
        std::snprintf(buf, sizeof buf, "%02x", c);
        out += buf;
      }
    } else {
      std::snprintf(buf, sizeof buf, "%lld", (long long)iv);
      out += buf;
    }
    out += "\n";
  };
  for (const RowGroup& rg : meta.row_groups) {
    for (const ColumnChunk& cc : rg.cols) {
      if (cc.path != leaf_name) continue;
      const HostColumn col = decode_column_host(file.data(), file.size(), cc, *leaf);
      const std::vector<Entry> sparse = sparse_entries(file.data(), file.size(), cc, *leaf, 0, row_base);
      if (sparse.size() != col.def.size()) dr::fail(DR_E_INTERNAL, "the two host decoders disagree on the level count");
      size_t vi = 0;
      for (size_t i = 0; i < col.def.size(); ++i) {
        const bool has = int(col.def[i]) == leaf->max_def;
        const int64_t iv = has && leaf->type != BYTE_ARRAY ? col.ivals.at(vi) : 0;
        const std::string sv = has && leaf->type == BYTE_ARRAY ? col.svals.at(vi) : std::string();
        vi += has;
        const Entry& e = sparse[i];
        if (e.def != col.def[i] || e.rep != col.rep[i] || e.has_value != has ||
            (has && (leaf->type == BYTE_ARRAY ? e.sval != sv : e.ival != iv)))
          dr::fail(DR_E_INTERNAL, "the two host decoders disagree on a value");
        put(col.def[i], col.rep[i], has, iv, sv);
      }
      levels += col.def.size();
    }
    row_base += rg.num_rows;
  }
  std::printf("leaf %s\nlevels %zu\n%sok\n", leaf_name.c_str(), levels, out.c_str());
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s FILE LEAF...\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  try {
    const FileMeta meta = parse_footer(file.data(), file.size());
    for (int ai = 2; ai < argc; ++ai) print_leaf(file, meta, argv[ai]);
  } catch (const dr::Error& e) {
    if (e.status == DR_E_PARQUET) std::fprintf(stderr, "DR_E_PARQUET: %s\n", e.what());
    else std::fprintf(stderr, "DR_E_%d: %s\n", e.status, e.what());
    return 3;
  }
  return 0;
}
