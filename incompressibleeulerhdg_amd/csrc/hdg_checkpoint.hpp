// Checkpoint blob of an engine: the digest formula, the writer, the reader and the validator.
// Plain C++, no HIP: the engine (hdg_engine.hip) decides WHAT a section is and moves device memory; everything that touches
// the bytes of a blob is here and is checked on the host by tests/host/checkpoint_check.cpp.
//
// Layout (little-endian, every part starts on a multiple of 8 bytes):
//   Header        64 bytes: magic, version, section count, step, t, total bytes, fingerprint bytes, and what a binding
//                 needs to resume the recorders: the numbers of probe points and particles, flags of what was switched on
//   fingerprint   text, one "name=value\n" line per field, zero-padded to a multiple of 8
//   section table 64 bytes per section: id, kind, length, offset (from the start of the blob), digest
//   payload       the sections in table order, each zero-padded to a multiple of 8
// Digest of n 64-bit words b_i:  d0 = sum b_i,  d1 = sum b_i (2 i + 1), both mod 2^64.  Integer sums are exact in any order, so
// the device kernel (k_digest) and digest_words below agree bit for bit whatever the grid; the odd weights make one changed
// word, or two unequal words exchanged, change d1.  Host bytes are digested as words after zero-padding the last one.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace hdg {
namespace ckpt {

struct Digest {
  uint64_t d0 = 0, d1 = 0;
  bool operator==(const Digest& o) const { return d0 == o.d0 && d1 == o.d1; }
  bool operator!=(const Digest& o) const { return !(*this == o); }
};

// p need not be aligned (a payload inside a caller's buffer)
inline Digest digest_words(const void* p, uint64_t nwords) {
  Digest d;
  const unsigned char* c = static_cast<const unsigned char*>(p);
  for (uint64_t i = 0; i < nwords; i++) {
    uint64_t b;
    std::memcpy(&b, c + 8 * i, 8);
    d.d0 += b;
    d.d1 += b * (2 * i + 1);
  }
  return d;
}
inline Digest digest_bytes(const void* p, uint64_t nbytes) {
  Digest d = digest_words(p, nbytes / 8);
  if (nbytes % 8) {
    uint64_t b = 0;
    std::memcpy(&b, static_cast<const unsigned char*>(p) + (nbytes / 8) * 8, nbytes % 8);
    d.d0 += b;
    d.d1 += b * (2 * (nbytes / 8) + 1);
  }
  return d;
}
// the digest of a list of digests, in order (hdg_state_digest)
inline Digest digest_of_digests(const std::vector<Digest>& v) {
  std::vector<uint64_t> w;
  for (const Digest& d : v) { w.push_back(d.d0); w.push_back(d.d1); }
  return digest_words(w.data(), w.size());
}

static constexpr char MAGIC[8] = {'H', 'D', 'G', 'C', 'K', 'P', 'T', '\0'};
static constexpr uint32_t VERSION = 1;
enum Kind : uint32_t { DEVICE_DOUBLES = 0, HOST_BYTES = 1 };
enum Flags : uint64_t { FLAG_TRACER = 1, FLAG_DIAGNOSTICS = 2, FLAG_PROBES = 4, FLAG_PARTICLES = 8 };

struct Header {
  char magic[8];
  uint32_t version;
  uint32_t n_sections;
  int64_t step;
  double t;
  uint64_t total_bytes;
  uint64_t fingerprint_bytes;  // unpadded
  int32_t n_probes;
  int32_t n_particles;
  uint64_t flags;  // FLAG_*: what the saved run had switched on
};
static_assert(sizeof(Header) == 64, "blob header is 64 bytes");

struct TableEntry {
  char id[24];      // zero-terminated
  uint32_t kind;
  uint32_t pad;
  uint64_t length;  // doubles (DEVICE_DOUBLES) or bytes (HOST_BYTES)
  uint64_t offset;  // of the payload, from the start of the blob
  uint64_t d0, d1;
};
static_assert(sizeof(TableEntry) == 64, "table entry is 64 bytes");

struct Section {
  std::string id;
  uint32_t kind = DEVICE_DOUBLES;
  uint64_t length = 0;
  uint64_t offset = 0;
  Digest digest;
  uint64_t bytes() const { return kind == DEVICE_DOUBLES ? 8 * length : length; }
};

inline uint64_t pad8(uint64_t n) { return (n + 7) & ~uint64_t(7); }

// ---- fingerprint: an ordered list of (name, value) pairs, compared field by field so that a refusal can name the field
struct Fingerprint {
  std::vector<std::pair<std::string, std::string>> f;
  void add(const std::string& name, long v) { f.emplace_back(name, std::to_string(v)); }
  void add_u64(const std::string& name, uint64_t v) {
    char b[32];
    snprintf(b, sizeof(b), "%016llx", (unsigned long long)v);
    f.emplace_back(name, b);
  }
  void add(const std::string& name, double v) {  // the bit pattern decides (no rounding through text), the number is for people
    uint64_t b;
    std::memcpy(&b, &v, 8);
    char s[64];
    snprintf(s, sizeof(s), "%016llx(%.17g)", (unsigned long long)b, v);
    f.emplace_back(name, s);
  }
  std::string text() const {
    std::string s;
    for (const auto& p : f) s += p.first + "=" + p.second + "\n";
    return s;
  }
  static Fingerprint parse(const std::string& s) {
    Fingerprint fp;
    size_t pos = 0;
    while (pos < s.size()) {
      size_t nl = s.find('\n', pos);
      if (nl == std::string::npos) nl = s.size();
      const std::string line = s.substr(pos, nl - pos);
      const size_t eq = line.find('=');
      if (eq != std::string::npos) fp.f.emplace_back(line.substr(0, eq), line.substr(eq + 1));
      pos = nl + 1;
    }
    return fp;
  }
  // empty: equal; otherwise the message that names the first field that differs
  std::string difference(const Fingerprint& file) const {
    const size_t n = std::min(f.size(), file.f.size());
    for (size_t i = 0; i < n; i++) {
      if (f[i].first != file.f[i].first)
        return "fingerprint field " + std::to_string(i) + " is '" + file.f[i].first + "' in the checkpoint and '" + f[i].first + "' in this engine";
      if (f[i].second != file.f[i].second)
        return "fingerprint field '" + f[i].first + "' differs: checkpoint " + file.f[i].second + ", this engine " + f[i].second;
    }
    if (f.size() != file.f.size())
      return "fingerprint has " + std::to_string(file.f.size()) + " fields in the checkpoint and " + std::to_string(f.size()) + " in this engine";
    return "";
  }
};

// ---- writer: lay the blob out (offsets into `sections`), then write header, fingerprint and table; the caller fills the
// payloads at their offsets and the digests before write_front
inline uint64_t layout(const std::string& fingerprint, std::vector<Section>& sections) {
  uint64_t off = sizeof(Header) + pad8(fingerprint.size()) + sizeof(TableEntry) * sections.size();
  for (Section& s : sections) { s.offset = off; off += pad8(s.bytes()); }
  return off;
}
inline void write_front(void* buf, uint64_t total, long step, double t, int n_probes, int n_particles, uint64_t flags, const std::string& fingerprint,
                        const std::vector<Section>& sections) {
  unsigned char* c = static_cast<unsigned char*>(buf);
  Header h;
  std::memset(&h, 0, sizeof(h));
  std::memcpy(h.magic, MAGIC, 8);
  h.version = VERSION;
  h.n_sections = (uint32_t)sections.size();
  h.step = step; h.t = t; h.total_bytes = total; h.fingerprint_bytes = fingerprint.size();
  h.n_probes = n_probes; h.n_particles = n_particles; h.flags = flags;
  std::memcpy(c, &h, sizeof(h));
  std::memset(c + sizeof(h), 0, pad8(fingerprint.size()));
  std::memcpy(c + sizeof(h), fingerprint.data(), fingerprint.size());
  unsigned char* tb = c + sizeof(h) + pad8(fingerprint.size());
  for (size_t i = 0; i < sections.size(); i++) {
    const Section& s = sections[i];
    TableEntry e;
    std::memset(&e, 0, sizeof(e));
    std::strncpy(e.id, s.id.c_str(), sizeof(e.id) - 1);
    e.kind = s.kind; e.length = s.length; e.offset = s.offset; e.d0 = s.digest.d0; e.d1 = s.digest.d1;
    std::memcpy(tb + sizeof(e) * i, &e, sizeof(e));
    const uint64_t b = s.bytes();
    if (pad8(b) != b) std::memset(c + s.offset + b, 0, pad8(b) - b);  // the padding of a host section
  }
}

// ---- reader and validator: never reads beyond buf + nbytes; empty return = a well-formed blob whose every payload matches
// the digest in its table entry.  Otherwise the message (magic, version, byte count, table bounds, the section by name).
struct Parsed {
  Header header;
  std::string fingerprint;
  std::vector<Section> sections;
};
inline std::string parse(const void* buf, uint64_t nbytes, Parsed& out, bool check_digests = true) {
  const unsigned char* c = static_cast<const unsigned char*>(buf);
  if (!buf) return "no buffer";
  if (nbytes < sizeof(Header))
    return "truncated: " + std::to_string(nbytes) + " bytes hold no header (" + std::to_string(sizeof(Header)) + " bytes)";
  Header& h = out.header;
  std::memcpy(&h, c, sizeof(h));
  if (std::memcmp(h.magic, MAGIC, 8) != 0) return "bad magic: not a checkpoint of this engine";
  if (h.version != VERSION)
    return "format version " + std::to_string(h.version) + " is not the version " + std::to_string(VERSION) + " this library reads";
  if (h.total_bytes != nbytes)
    return "byte count: the checkpoint says " + std::to_string(h.total_bytes) + " bytes, " + std::to_string(nbytes) + " were given (truncated?)";
  uint64_t off = sizeof(Header);
  if (h.fingerprint_bytes > nbytes - off || pad8(h.fingerprint_bytes) > nbytes - off) return "fingerprint leaves the blob";
  out.fingerprint.assign(reinterpret_cast<const char*>(c + off), (size_t)h.fingerprint_bytes);
  off += pad8(h.fingerprint_bytes);
  if ((uint64_t)h.n_sections > (nbytes - off) / sizeof(TableEntry)) return "section table leaves the blob";
  const uint64_t payload0 = off + sizeof(TableEntry) * (uint64_t)h.n_sections;
  out.sections.clear();
  for (uint32_t i = 0; i < h.n_sections; i++) {
    TableEntry e;
    std::memcpy(&e, c + off + sizeof(e) * i, sizeof(e));
    e.id[sizeof(e.id) - 1] = 0;
    Section s;
    s.id = e.id; s.kind = e.kind; s.length = e.length; s.offset = e.offset; s.digest.d0 = e.d0; s.digest.d1 = e.d1;
    if (s.kind != DEVICE_DOUBLES && s.kind != HOST_BYTES) return "section '" + s.id + "': unknown kind " + std::to_string(s.kind);
    if (s.kind == DEVICE_DOUBLES && s.length > (UINT64_MAX >> 3)) return "section '" + s.id + "': length overflows";
    const uint64_t b = s.bytes();
    if (s.offset % 8 != 0 || s.offset < payload0 || s.offset > nbytes || b > nbytes - s.offset)
      return "section '" + s.id + "': offset " + std::to_string(s.offset) + " + " + std::to_string(b) + " bytes leave the blob of " +
             std::to_string(nbytes) + " bytes";
    out.sections.push_back(s);
  }
  if (check_digests)
    for (const Section& s : out.sections) {
      const Digest d = s.kind == DEVICE_DOUBLES ? digest_words(c + s.offset, s.length) : digest_bytes(c + s.offset, s.length);
      if (d != s.digest) return "section '" + s.id + "': the bytes do not match the digest in the table (corrupted checkpoint)";
    }
  return "";
}

// ---- host sections are flat records written and read through these two
struct ByteWriter {
  std::vector<unsigned char> b;
  void raw(const void* p, size_t n) { const unsigned char* c = static_cast<const unsigned char*>(p); b.insert(b.end(), c, c + n); }
  template <class T> void put(const T& v) { raw(&v, sizeof(T)); }
  template <class T> void vec(const std::vector<T>& v) { put<uint64_t>(v.size()); if (!v.empty()) raw(v.data(), sizeof(T) * v.size()); }
};
struct ByteReader {
  const unsigned char* p;
  size_t n, pos = 0;
  bool ok = true;
  ByteReader(const void* p_, size_t n_) : p(static_cast<const unsigned char*>(p_)), n(n_) {}
  void raw(void* out, size_t k) {
    if (!ok || k > n - pos) { ok = false; std::memset(out, 0, k); return; }
    std::memcpy(out, p + pos, k);
    pos += k;
  }
  template <class T> T get() { T v; raw(&v, sizeof(T)); return v; }
  template <class T> void vec(std::vector<T>& v) {
    const uint64_t k = get<uint64_t>();
    if (!ok || k > (n - pos) / sizeof(T)) { ok = false; v.clear(); return; }
    v.resize((size_t)k);
    if (k) raw(v.data(), sizeof(T) * (size_t)k);
  }
  bool done() const { return ok && pos == n; }
};

}  // namespace ckpt
}  // namespace hdg
