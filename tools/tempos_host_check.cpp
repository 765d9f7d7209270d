// Host-side check of the tempo stream's arithmetic and argument checks (include/sparkmi.h, smi_tempos_*), for a sanitizer build
// on a machine without a GPU.  A stand-alone program, from spark-tts_amd/csrc:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -I../../include -I. -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined ../../tools/tempos_host_check.cpp smi_audio.hip smi_core.hip -o tempos_host_check
// It walks smi_tempos_piece_len over streams cut at random, against the definition written out here; checks that the pieces sum
// to M and that the history bound holds; and sends every call the arguments it must refuse before it touches a device.  What
// needs a device -- a created handle, hence the per-row checks and the switching of sets in smi_tempos_push_rows -- is covered
// by tests/test_tempo_stream_gpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sparkmi.h"

static long long nominal(long long k, int p, int q, int H) { return k * H * p / q; }

static long long ready(long long k, int p, int q, int N, int D) {
  const int H = N / 2;
  if (k == 0) return H;
  const long long a = nominal(k, p, q, H), b = nominal(k - 1, p, q, H) + H;
  return (a > b ? a : b) + D + N;
}

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);           \
      return 1;                                                      \
    }                                                                \
  } while (0)

int main() {
  const int tempos[][2] = {{5, 4}, {4, 5}, {2, 1}, {1, 2}, {3, 2}, {101, 100}, {99, 100}, {4, 1}, {1, 4}, {1, 1}};
  const int frames[][2] = {{16, 4}, {16, 0}, {64, 8}, {512, 240}, {2048, 1024}};
  uint64_t rng = 88172645463325252ull;
  auto next = [&rng](long long m) {
    rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
    return (long long)(rng % (uint64_t)m);
  };
  long long pushes = 0;
  for (const auto& t : tempos)
    for (const auto& f : frames) {
      const int p = t[0], q = t[1], N = f[0], D = f[1], H = N / 2;
      const long long cap = 7LL * H + D > 5LL * H + 2LL * D ? 7LL * H + D : 5LL * H + 2LL * D;
      for (int trial = 0; trial < 20; ++trial) {
        const long long L = next(20LL * N + 38);
        long long n = 0, fr = 0, sum = 0;
        while (true) {
          const long long len = n == L ? 0 : next(L - n + 1);
          const int last = n + len == L && next(2);
          long long n2 = -7, f2 = -7;
          const long long piece = smi_tempos_piece_len(p, q, N, D, n, fr, len, last, &n2, &f2);
          CHECK(piece >= 0 && n2 == n + len);
          const long long M = (n2 * q + p - 1) / p;
          long long want_f = 0;
          if (last) want_f = M ? (M - 1) / H + 1 : 0;
          else if (p == q) want_f = n2 / H;
          else
            while ((want_f + 1) * H <= M && n2 >= ready(want_f, p, q, N, D)) ++want_f;
          CHECK(f2 == want_f);
          CHECK(piece == (p == q ? len : last ? M - fr * H : (f2 - fr) * H));
          if (!last && p != q) {   // the history the next frame can still read
            long long h0 = 0;
            if (f2) {
              const long long a = nominal(f2, p, q, H), b = nominal(f2 - 1, p, q, H) + H;
              h0 = (a < b ? a : b) - D;
              if (h0 < 0) h0 = 0;
            }
            CHECK(n2 - h0 <= cap);
          }
          sum += piece;
          n = n2; fr = f2;
          ++pushes;
          if (last) break;
        }
        CHECK(sum == (L * q + p - 1) / p);
      }
    }
  // what the arithmetic refuses
  CHECK(smi_tempos_piece_len(5, 1, 64, 8, 0, 0, 10, 0, nullptr, nullptr) == -1);
  CHECK(smi_tempos_piece_len(0, 1, 64, 8, 0, 0, 10, 0, nullptr, nullptr) == -1);
  CHECK(smi_tempos_piece_len(5, 4, 63, 8, 0, 0, 10, 0, nullptr, nullptr) == -1);
  CHECK(smi_tempos_piece_len(5, 4, 64, 1025, 0, 0, 10, 0, nullptr, nullptr) == -1);
  CHECK(smi_tempos_piece_len(5, 4, 64, 8, -1, 0, 10, 0, nullptr, nullptr) == -1);
  CHECK(smi_tempos_piece_len(5, 4, 64, 8, 0, 0, -1, 0, nullptr, nullptr) == -1);
  CHECK(smi_tempos_piece_len(5, 4, 64, 8, 0, 0, 10, 2, nullptr, nullptr) == -1);
  CHECK(smi_tempos_piece_len(5, 4, 64, 8, 10, 4000, 10, 1, nullptr, nullptr) == -1);
  CHECK(smi_tempos_piece_len(5, 4, 64, 8, 1LL << 40, 0, 10, 0, nullptr, nullptr) == -1);
  // what the calls refuse before they touch a device
  double win[16] = {0};
  smi_tempos* h = nullptr;
  CHECK(smi_tempos_create(1, 100, 16, 4, win, nullptr) == SMI_EINVAL);
  CHECK(smi_tempos_create(0, 100, 16, 4, win, &h) == SMI_EINVAL && std::strstr(smi_last_error(), "max_streams") && !h);
  CHECK(smi_tempos_create(1, 0, 16, 4, win, &h) == SMI_EINVAL && std::strstr(smi_last_error(), "max_chunk"));
  CHECK(smi_tempos_create(1, 100, 18 + 1, 4, win, &h) == SMI_EINVAL && std::strstr(smi_last_error(), "N="));
  CHECK(smi_tempos_create(1, 100, 16, -1, win, &h) == SMI_EINVAL && std::strstr(smi_last_error(), "D="));
  CHECK(smi_tempos_create(1, 100, 16, 4, nullptr, &h) == SMI_EINVAL && std::strstr(smi_last_error(), "win_host"));
  CHECK(smi_tempos_open(nullptr, 0, 5, 4) == SMI_EINVAL);
  int32_t one[1] = {0};
  float x[1] = {0};
  CHECK(smi_tempos_push_rows(nullptr, x, 1, one, one, one, 1, nullptr, 0, x, 1, nullptr, nullptr) == SMI_EINVAL);
  CHECK(smi_tempos_destroy(nullptr) == SMI_OK);
  std::printf("tempos host check ok: %lld pushes\n", pushes);
  return 0;
}
