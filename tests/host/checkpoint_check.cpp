// Host check of csrc/hdg_checkpoint.hpp (plain C++; built with -fsanitize=address,undefined by tests/test_checkpoint_cpu.py):
// round trip of a synthetic blob, every truncation, table entries that leave the file, bad magic and version, one flipped
// byte named by its section, the fingerprint's naming of the field that differs, and the digest of fixed words, printed for
// the comparison with tests/checkpoint_reference.py.  Every buffer handed to the reader is an exact-size heap copy, so a read
// past the end is an AddressSanitizer error.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../../incompressibleeulerhdg_amd/csrc/hdg_checkpoint.hpp"

using namespace hdg::ckpt;

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } \
  } while (0)

static std::vector<uint64_t> fixed_words(size_t n) {
  std::vector<uint64_t> w(n);
  uint64_t x = 88172645463325252ULL;
  for (size_t i = 0; i < n; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; w[i] = x; }
  return w;
}
// parse an exact-size heap copy of the first n bytes
static std::string parse_copy(const std::vector<unsigned char>& blob, size_t n, Parsed& P) {
  std::unique_ptr<unsigned char[]> c(new unsigned char[n ? n : 1]);
  if (n) std::memcpy(c.get(), blob.data(), n);
  return parse(n ? c.get() : c.get(), n, P);
}

int main() {
  // ---- digests of fixed words (compared with numpy by the test) and the properties the odd weights give
  for (size_t n : {0, 1, 2, 5, 64, 1000}) {
    const std::vector<uint64_t> w = fixed_words(n);
    const Digest d = digest_words(w.data(), n);
    printf("digest %zu %llu %llu\n", n, (unsigned long long)d.d0, (unsigned long long)d.d1);
  }
  {
    std::vector<uint64_t> w = fixed_words(100);
    const Digest d = digest_words(w.data(), w.size());
    std::swap(w[3], w[77]);
    const Digest e = digest_words(w.data(), w.size());
    CHECK(e.d0 == d.d0 && e.d1 != d.d1);  // a swap of unequal words: visible in d1 only
    w[10] ^= 1ULL << 40;
    CHECK(digest_words(w.data(), w.size()).d0 != e.d0);
    const unsigned char bytes[11] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    const uint64_t two[2] = {0x0807060504030201ULL, 0x00000000000b0a09ULL};
    CHECK(digest_bytes(bytes, 11) == digest_words(two, 2));
    const Digest b = digest_bytes(bytes, 11);
    printf("digest_bytes 11 %llu %llu\n", (unsigned long long)b.d0, (unsigned long long)b.d1);
    CHECK(digest_of_digests({d, e}) == digest_words(std::vector<uint64_t>{d.d0, d.d1, e.d0, e.d1}.data(), 4));
  }
  // ---- a synthetic blob: two device sections and a host section of odd length
  Fingerprint fp;
  fp.add("degree", 2L); fp.add("dt", 0.0078125); fp.add_u64("cells_d0", 0xdeadbeefULL);
  const std::string fpt = fp.text();
  std::vector<Section> secs(3);
  const std::vector<uint64_t> a = fixed_words(37), b = fixed_words(8);
  const unsigned char host[13] = {9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 1, 2, 3};
  secs[0].id = "curQ"; secs[0].kind = DEVICE_DOUBLES; secs[0].length = a.size(); secs[0].digest = digest_words(a.data(), a.size());
  secs[1].id = "recL"; secs[1].kind = DEVICE_DOUBLES; secs[1].length = b.size(); secs[1].digest = digest_words(b.data(), b.size());
  secs[2].id = "solver"; secs[2].kind = HOST_BYTES; secs[2].length = sizeof(host); secs[2].digest = digest_bytes(host, sizeof(host));
  const uint64_t total = layout(fpt, secs);
  CHECK(total % 8 == 0 && secs[0].offset % 8 == 0 && secs[2].offset + 16 == total);
  std::vector<unsigned char> blob((size_t)total, 0xAB);
  std::memcpy(blob.data() + secs[0].offset, a.data(), 8 * a.size());
  std::memcpy(blob.data() + secs[1].offset, b.data(), 8 * b.size());
  std::memcpy(blob.data() + secs[2].offset, host, sizeof(host));
  write_front(blob.data(), total, 123456789012L, 0.375, 8, 64, FLAG_TRACER | FLAG_PROBES, fpt, secs);
  {
    Parsed P;
    const std::string err = parse_copy(blob, blob.size(), P);
    CHECK(err.empty());
    CHECK(P.header.step == 123456789012L && P.header.t == 0.375 && P.header.n_probes == 8 && P.header.n_particles == 64);
    CHECK(P.header.flags == (FLAG_TRACER | FLAG_PROBES));
    CHECK(P.fingerprint == fpt && P.sections.size() == 3);
    for (size_t i = 0; i < 3 && i < P.sections.size(); i++)
      CHECK(P.sections[i].id == secs[i].id && P.sections[i].length == secs[i].length && P.sections[i].offset == secs[i].offset &&
            P.sections[i].digest == secs[i].digest && P.sections[i].kind == secs[i].kind);
    CHECK(fp.difference(Fingerprint::parse(P.fingerprint)).empty());
    Fingerprint other;
    other.add("degree", 3L); other.add("dt", 0.0078125); other.add_u64("cells_d0", 0xdeadbeefULL);
    CHECK(other.difference(Fingerprint::parse(P.fingerprint)).find("'degree'") != std::string::npos);
    Fingerprint other2;
    other2.add("degree", 2L); other2.add("dt", 0.0078125000000000017); other2.add_u64("cells_d0", 0xdeadbeefULL);
    CHECK(other2.difference(Fingerprint::parse(P.fingerprint)).find("'dt'") != std::string::npos);  // one unit in the last place
  }
  // ---- every truncation is an error, and reads nothing past its end
  size_t refused = 0;
  for (size_t n = 0; n < blob.size(); n++) {
    Parsed P;
    if (!parse_copy(blob, n, P).empty()) refused++;
  }
  CHECK(refused == blob.size());
  printf("truncations refused %zu of %zu\n", refused, blob.size());
  {  // ... also when the header is made to agree with the shorter length
    for (size_t n = sizeof(Header); n < blob.size(); n += 8) {
      std::vector<unsigned char> cut(blob.begin(), blob.begin() + (long)n);
      Header h;
      std::memcpy(&h, cut.data(), sizeof(h));
      h.total_bytes = n;
      std::memcpy(cut.data(), &h, sizeof(h));
      Parsed P;
      CHECK(!parse_copy(cut, cut.size(), P).empty());
    }
  }
  // ---- table entries whose offset + length leave the file
  const size_t table0 = sizeof(Header) + (size_t)pad8(fpt.size());
  for (int variant = 0; variant < 5; variant++) {
    std::vector<unsigned char> bad = blob;
    TableEntry e;
    std::memcpy(&e, bad.data() + table0 + sizeof(e), sizeof(e));  // entry 1
    if (variant == 0) e.length = (total - e.offset) / 8 + 1;
    if (variant == 1) e.offset = total;
    if (variant == 2) e.length = UINT64_MAX / 4;   // 8 * length wraps
    if (variant == 3) e.offset = UINT64_MAX - 7;   // offset + bytes wraps
    if (variant == 4) e.offset = 8;                // inside the header
    std::memcpy(bad.data() + table0 + sizeof(e), &e, sizeof(e));
    Parsed P;
    const std::string err = parse_copy(bad, bad.size(), P);
    CHECK(err.find("'recL'") != std::string::npos);
  }
  {
    std::vector<unsigned char> bad = blob;
    Header h;
    std::memcpy(&h, bad.data(), sizeof(h));
    h.n_sections = 0x7fffffff;
    std::memcpy(bad.data(), &h, sizeof(h));
    Parsed P;
    CHECK(parse_copy(bad, bad.size(), P).find("section table") != std::string::npos);
    h.n_sections = 3; h.fingerprint_bytes = UINT64_MAX - 3;
    std::memcpy(bad.data(), &h, sizeof(h));
    CHECK(parse_copy(bad, bad.size(), P).find("fingerprint") != std::string::npos);
  }
  // ---- magic, version, one flipped payload byte
  {
    std::vector<unsigned char> bad = blob;
    bad[0] ^= 0x20;
    Parsed P;
    CHECK(parse_copy(bad, bad.size(), P).find("magic") != std::string::npos);
    bad = blob;
    bad[8] = 2;  // version
    CHECK(parse_copy(bad, bad.size(), P).find("version 2") != std::string::npos);
    for (size_t i = 0; i < 3; i++) {
      bad = blob;
      bad[(size_t)secs[i].offset + (size_t)secs[i].bytes() - 1] ^= 0x01;
      CHECK(parse_copy(bad, bad.size(), P).find("'" + secs[i].id + "'") != std::string::npos);
    }
  }
  // ---- the flat records of the host sections
  {
    ByteWriter w;
    w.vec(std::vector<double>{1.5, -2.5}); w.put<int>(7); w.vec(std::vector<char>{});
    std::vector<double> v; std::vector<char> c;
    ByteReader r(w.b.data(), w.b.size());
    r.vec(v); const int i = r.get<int>(); r.vec(c);
    CHECK(r.done() && v.size() == 2 && v[1] == -2.5 && i == 7 && c.empty());
    for (size_t n = 0; n < w.b.size(); n++) {  // every shorter record fails, none reads past its end
      std::unique_ptr<unsigned char[]> cp(new unsigned char[n ? n : 1]);
      if (n) std::memcpy(cp.get(), w.b.data(), n);
      ByteReader q(cp.get(), n);
      q.vec(v); (void)q.get<int>(); q.vec(c);
      CHECK(!q.done());
    }
    unsigned char huge[8];
    const uint64_t big = UINT64_MAX;
    std::memcpy(huge, &big, 8);
    ByteReader q(huge, 8);
    q.vec(v);
    CHECK(!q.ok && v.empty());
  }
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
