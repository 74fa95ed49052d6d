// CPU driver of `make san_wav`: svt_wav_parse and svt_wav_header (csrc/host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer.
//   wav_san_test <seed> <mutations> <file>...
// Every file is parsed whole, then as a prefix cut at every length (the need-more protocol) and as a FILE cut at every length (the
// truncations), each time from a heap buffer of exactly that size, so one byte read past the prefix is a finding; then `mutations` seeded
// single- and double-byte changes of each file's first 128 bytes are parsed.  The driver itself asserts only: the return code is one of
// SVT_OK / SVT_WAV_NEED_MORE / SVT_ERR_INVALID, `out` is untouched unless the code is SVT_OK, a request for more names a longer prefix
// inside the file, an accepted header describes frames that lie inside the file, and a refusal's text begins "svt_wav_parse".  The
// header writer is run into exact-size buffers and parsed back.  tests/test_wav_sanitizers.py builds and runs it as a child process.
#include "../../include/svt_mi355.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static long g_calls = 0, g_ok = 0, g_more = 0, g_refused = 0;

#define REQUIRE(cond, ...)                                   \
  do {                                                       \
    if (!(cond)) {                                           \
      std::fprintf(stderr, "wav_san_driver: " __VA_ARGS__);  \
      std::fprintf(stderr, " [%s]\n", #cond);                \
      std::exit(2);                                          \
    }                                                        \
  } while (0)

// one call on an exact-size heap copy of data[0, head_bytes)
static int parse_checked(const unsigned char* data, int64_t head_bytes, int64_t file_bytes, svt_wav_info* result) {
  unsigned char* head = (unsigned char*)std::malloc(head_bytes > 0 ? (size_t)head_bytes : 1);
  if (head_bytes > 0) std::memcpy(head, data, (size_t)head_bytes);
  svt_wav_info before, out;
  std::memset(&before, 0x5A, sizeof(before));
  std::memcpy(&out, &before, sizeof(out));
  int64_t need = -12345;
  const int rc = svt_wav_parse(head_bytes > 0 ? head : nullptr, head_bytes, file_bytes, &out, &need);
  std::free(head);
  ++g_calls;
  REQUIRE(rc == SVT_OK || rc == SVT_WAV_NEED_MORE || rc == SVT_ERR_INVALID, "return code %d", rc);
  if (rc == SVT_OK) {
    ++g_ok;
    REQUIRE(out.format >= SVT_PCM_U8 && out.format <= SVT_PCM_F64 && out.channels >= 1 && out.channels <= 8 && out.sample_rate >= 1, "fields");
    REQUIRE(out.block_align == out.channels * out.bits_per_sample / 8 && out.block_align >= 1, "block_align");
    REQUIRE(out.data_offset >= 20 && out.data_offset <= file_bytes && out.data_offset <= head_bytes, "data_offset %lld", (long long)out.data_offset);
    REQUIRE(out.frames >= 0 && out.frames <= (file_bytes - out.data_offset) / out.block_align, "frames %lld", (long long)out.frames);
  } else {
    REQUIRE(std::memcmp(&out, &before, sizeof(out)) == 0, "out was written with return code %d", rc);
    if (rc == SVT_WAV_NEED_MORE) {
      ++g_more;
      REQUIRE(need > head_bytes && need <= file_bytes, "need_bytes %lld for a prefix of %lld of %lld", (long long)need, (long long)head_bytes, (long long)file_bytes);
    } else {
      ++g_refused;
      REQUIRE(std::strncmp(svt_last_error(), "svt_wav_parse", 13) == 0, "error text '%s'", svt_last_error());
    }
  }
  if (result) *result = out;
  return rc;
}

static std::vector<unsigned char> read_file(const char* path) {
  std::vector<unsigned char> v;
  FILE* f = std::fopen(path, "rb");
  REQUIRE(f != nullptr, "cannot open %s", path);
  unsigned char buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return v;
}

static uint64_t g_state;
static uint32_t rnd() {   // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static void headers() {
  for (int fmt : {(int)SVT_PCM_S16, (int)SVT_PCM_F32}) {
    const int64_t size = fmt == SVT_PCM_S16 ? 44 : 58;
    for (int ch = 1; ch <= 8; ++ch) {
      for (int64_t frames : {(int64_t)0, (int64_t)1, (int64_t)48000, (int64_t)((0xFFFFFFFFll - size) / (ch * (fmt == SVT_PCM_S16 ? 2 : 4)))}) {
        unsigned char* buf = (unsigned char*)std::malloc((size_t)size);
        int64_t n = -1;
        REQUIRE(svt_wav_header(fmt, ch, 44100, frames, buf, size, &n) == SVT_OK && n == size, "svt_wav_header: %s", svt_last_error());
        svt_wav_info wi;
        const int64_t align = ch * (fmt == SVT_PCM_S16 ? 2 : 4);
        REQUIRE(parse_checked(buf, size, size + frames * align, &wi) == SVT_OK, "round trip: %s", svt_last_error());
        REQUIRE(wi.format == fmt && wi.channels == ch && wi.sample_rate == 44100 && wi.frames == frames && wi.data_offset == size && wi.block_align == align, "round trip fields");
        REQUIRE(svt_wav_header(fmt, ch, 44100, frames, buf, size - 1, &n) == SVT_ERR_INVALID, "a short buffer must be refused");
        REQUIRE(svt_wav_header(fmt, ch, 44100, (0xFFFFFFFFll - size) / align + 1, buf, size, &n) == SVT_ERR_INVALID, "too much data must be refused");
        std::free(buf);
      }
    }
  }
  unsigned char buf[64];
  int64_t n = -1;
  REQUIRE(svt_wav_header(SVT_PCM_S24, 2, 44100, 1, buf, 64, &n) == SVT_ERR_INVALID && svt_wav_header(SVT_PCM_S16, 9, 44100, 1, buf, 64, &n) == SVT_ERR_INVALID &&
          svt_wav_header(SVT_PCM_S16, 2, 0, 1, buf, 64, &n) == SVT_ERR_INVALID && svt_wav_header(SVT_PCM_S16, 2, 44100, -1, buf, 64, &n) == SVT_ERR_INVALID &&
          svt_wav_header(SVT_PCM_S16, 2, 44100, 1, nullptr, 64, &n) == SVT_ERR_INVALID && svt_wav_header(SVT_PCM_S16, 2, 44100, 1, buf, 64, nullptr) == SVT_ERR_INVALID,
          "header refusals");
}

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s <seed> <mutations> <file>...\n", argv[0]); return 64; }
  g_state = std::strtoull(argv[1], nullptr, 10);
  const long mutations = std::strtol(argv[2], nullptr, 10);
  const int n_files = argc - 3;
  svt_wav_info wi;
  REQUIRE(svt_wav_parse(nullptr, 0, 0, nullptr, nullptr) == SVT_ERR_INVALID, "a null out must be refused");
  for (int k = 0; k < n_files; ++k) {
    const std::vector<unsigned char> file = read_file(argv[3 + k]);
    const int64_t len = (int64_t)file.size();
    const int whole = parse_checked(file.data(), len, len, &wi);
    REQUIRE(whole != SVT_WAV_NEED_MORE, "%s: a whole file cannot need more", argv[3 + k]);
    for (int64_t n = 0; n <= len; ++n) {
      svt_wav_info part;
      const int rc = parse_checked(file.data(), n, len, &part);                 // a prefix of the file
      if (whole == SVT_OK) {
        REQUIRE(rc == SVT_OK || rc == SVT_WAV_NEED_MORE, "%s: prefix %lld of a good file was refused", argv[3 + k], (long long)n);
        if (rc == SVT_OK) REQUIRE(std::memcmp(&part, &wi, sizeof(wi)) == 0, "%s: prefix %lld parses differently", argv[3 + k], (long long)n);
      }
      parse_checked(file.data(), n, n, nullptr);                                  // the file cut at n
    }
  }
  for (long m = 0; m < mutations; ++m) {
    std::vector<unsigned char> file = read_file(argv[3 + (int)(rnd() % (uint32_t)n_files)]);
    if (file.empty()) continue;
    const uint32_t span = file.size() < 128 ? (uint32_t)file.size() : 128u;
    const int changes = 1 + (int)(rnd() & 1);
    for (int c = 0; c < changes; ++c) {
      const uint32_t at = rnd() % span, how = rnd() % 4;
      file[at] = how == 0 ? (unsigned char)rnd() : how == 1 ? (unsigned char)(file[at] ^ (1u << (rnd() % 8))) : how == 2 ? 0xFF : 0x00;
    }
    const int64_t len = (int64_t)file.size();
    const int rc = parse_checked(file.data(), len, len, nullptr);
    REQUIRE(rc != SVT_WAV_NEED_MORE, "a whole file cannot need more");
    const int64_t cut = (int64_t)(rnd() % (uint32_t)(len + 1));
    parse_checked(file.data(), cut, len, nullptr);
  }
  headers();
  std::printf("wav ok: %ld calls, %ld parsed, %ld asked for more, %ld refused\n", g_calls, g_ok, g_more, g_refused);
  return 0;
}
