// Host-side check of the pitch stream's arithmetic and argument checks (include/sparkmi.h, smi_pitchs_*), for a sanitizer build
// on a machine without a GPU.  A stand-alone program, from spark-tts_amd/csrc:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -I../../include -I. -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined ../../tools/pitchs_host_check.cpp smi_audio.hip smi_core.hip -o pitchs_host_check
// It walks smi_pitchs_piece_len over streams cut at random, against the definition written out here (the stretch's counters come
// from smi_tempos_piece_len, which tools/tempos_host_check.cpp holds to its own definition); checks that K never falls, never
// passes ceil(n tq / tp) and that the pieces sum to n_out, and that the stretched tail stays within 2 G / up; and sends every
// call the arguments it must refuse before it touches a device.  What needs a device -- a created handle, hence open's checks,
// the per-row checks and the switching of sets in smi_pitchs_push_rows -- is covered by tests/test_pitch_stream_gpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sparkmi.h"

static long long gcd(long long a, long long b) {
  while (b) { const long long t = a % b; a = b; b = t; }
  return a;
}

static long long ceil_div(long long a, long long b) { return a <= 0 ? 0 : (a + b - 1) / b; }

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);           \
      return 1;                                                      \
    }                                                                \
  } while (0)

int main() {
  const int tempos[][2] = {{1, 1}, {5, 4}, {4, 5}, {2, 1}, {1, 2}, {3, 2}};
  const int ratios[][2] = {{3, 2}, {2, 3}, {28, 25}, {89, 100}, {199, 100}, {101, 200}, {2, 1}, {1, 2}, {1, 1}, {7, 7}};
  const int frames[][2] = {{16, 3}, {64, 8}, {512, 240}, {2048, 1024}};
  uint64_t rng = 88172645463325252ull;
  auto next = [&rng](long long m) {
    rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
    return (long long)(rng % (uint64_t)m);
  };
  long long pushes = 0, streams = 0;
  for (const auto& t : tempos)
    for (const auto& r : ratios)
      for (const auto& f : frames) {
        const int tp = t[0], tq = t[1], rp = r[0], rq = r[1], N = f[0], D = f[1], H = N / 2;
        const long long a = (long long)tp * rq, b = (long long)tq * rp, g = gcd(a, b), gr = gcd(rp, rq);
        const int P = (int)(a / g), Q = (int)(b / g), up = (int)(rq / gr), down = (int)(rp / gr);
        if (P > 4 * Q || Q > 4 * P) {   // no such stretch
          CHECK(smi_pitchs_piece_len(tp, tq, rp, rq, N, D, 0, 0, 0, 0, 10, 0, nullptr, nullptr, nullptr) == -1);
          continue;
        }
        const int G = up == 1 && down == 1 ? 0 : 10 * (up > down ? up : down), nt = G ? 2 * G + 1 : 0;
        ++streams;
        for (int trial = 0; trial < 12; ++trial) {
          const long long L = next(20LL * N + 38);
          long long n = 0, fr = 0, k = 0, sum = 0;
          while (true) {
            const long long len = n == L ? 0 : next(L - n + 1);
            const int last = n + len == L && next(2);
            long long n2 = -7, f2 = -7, k2 = -7, nt2 = -7, ft2 = -7;
            const long long piece = smi_pitchs_piece_len(tp, tq, rp, rq, N, D, nt, n, fr, k, len, last, &n2, &f2, &k2);
            CHECK(piece >= 0 && n2 == n + len && k2 == k + piece);
            CHECK(smi_tempos_piece_len(P, Q, N, D, n, fr, len, last, &nt2, &ft2) >= 0 && nt2 == n2 && ft2 == f2);
            const long long n_out = (n2 * tq + tp - 1) / tp, M = (n2 * Q + P - 1) / P;
            const long long E = last ? M : P == Q ? n2 : f2 * H;
            CHECK(k2 == (last ? n_out : ceil_div(E * up - G, down)));
            CHECK(k2 <= n_out);
            if (!last && G) {   // the stretched samples the outputs still to come reach
              const long long t0 = ceil_div(k2 * down - G, up);
              CHECK(t0 <= E && E - t0 <= 2LL * G / up && E - t0 <= nt + 1);
              CHECK(k2 == 0 || (k2 - 1) * down + G < E * up);   // the last emitted output's sum ends inside what is final
            }
            sum += piece;
            n = n2; fr = f2; k = k2;
            ++pushes;
            if (last) break;
          }
          CHECK(sum == (L * tq + tp - 1) / tp);
        }
      }
  // what the arithmetic refuses
  CHECK(smi_pitchs_piece_len(0, 1, 3, 2, 64, 8, 61, 0, 0, 0, 10, 0, nullptr, nullptr, nullptr) == -1);
  CHECK(smi_pitchs_piece_len(1, 1, 3, 40000, 64, 8, 61, 0, 0, 0, 10, 0, nullptr, nullptr, nullptr) == -1);
  CHECK(smi_pitchs_piece_len(1, 4, 4, 1, 64, 8, 81, 0, 0, 0, 10, 0, nullptr, nullptr, nullptr) == -1);
  CHECK(smi_pitchs_piece_len(1, 1, 3, 2, 63, 8, 61, 0, 0, 0, 10, 0, nullptr, nullptr, nullptr) == -1);
  CHECK(smi_pitchs_piece_len(1, 1, 3, 2, 64, 1025, 61, 0, 0, 0, 10, 0, nullptr, nullptr, nullptr) == -1);
  CHECK(smi_pitchs_piece_len(1, 1, 3, 2, 64, 8, 60, 0, 0, 0, 10, 0, nullptr, nullptr, nullptr) == -1);
  CHECK(smi_pitchs_piece_len(1, 1, 3, 2, 64, 8, 0, 0, 0, 0, 10, 0, nullptr, nullptr, nullptr) == -1);
  CHECK(smi_pitchs_piece_len(1, 1, 3, 2, 64, 8, 3, 0, 0, 0, 10, 0, nullptr, nullptr, nullptr) == -1);     // G = 1 < up = 2
  CHECK(smi_pitchs_piece_len(1, 1, 5, 5, 64, 8, 61, 0, 0, 0, 10, 0, nullptr, nullptr, nullptr) == -1);    // taps at 1/1
  CHECK(smi_pitchs_piece_len(1, 1, 3, 2, 64, 8, 61, -1, 0, 0, 10, 0, nullptr, nullptr, nullptr) == -1);
  CHECK(smi_pitchs_piece_len(1, 1, 3, 2, 64, 8, 61, 0, 0, -1, 10, 0, nullptr, nullptr, nullptr) == -1);
  CHECK(smi_pitchs_piece_len(1, 1, 3, 2, 64, 8, 61, 0, 0, 0, -1, 0, nullptr, nullptr, nullptr) == -1);
  CHECK(smi_pitchs_piece_len(1, 1, 3, 2, 64, 8, 61, 0, 0, 0, 10, 2, nullptr, nullptr, nullptr) == -1);
  CHECK(smi_pitchs_piece_len(1, 1, 3, 2, 64, 8, 61, 100, 0, 500, 10, 0, nullptr, nullptr, nullptr) == -1);
  CHECK(smi_pitchs_piece_len(1, 1, 3, 2, 64, 8, 61, 1LL << 40, 0, 0, 10, 0, nullptr, nullptr, nullptr) == -1);
  CHECK(smi_pitchs_piece_len(1, 1, 101, 200, 64, 8, 4001, 1LL << 27, 0, 0, 10, 1, nullptr, nullptr, nullptr) == -1);   // E up reaches 2^31
  // what the calls refuse before they touch a device
  double win[16] = {0};
  smi_pitchs* h = nullptr;
  CHECK(smi_pitchs_create(1, 100, 16, 3, win, 61, nullptr) == SMI_EINVAL);
  CHECK(smi_pitchs_create(0, 100, 16, 3, win, 61, &h) == SMI_EINVAL && std::strstr(smi_last_error(), "max_streams") && !h);
  CHECK(smi_pitchs_create(1, 0, 16, 3, win, 61, &h) == SMI_EINVAL && std::strstr(smi_last_error(), "max_chunk"));
  CHECK(smi_pitchs_create(1, 100, 18 + 1, 3, win, 61, &h) == SMI_EINVAL && std::strstr(smi_last_error(), "N="));
  CHECK(smi_pitchs_create(1, 100, 16, -1, win, 61, &h) == SMI_EINVAL && std::strstr(smi_last_error(), "D="));
  CHECK(smi_pitchs_create(1, 100, 16, 3, nullptr, 61, &h) == SMI_EINVAL && std::strstr(smi_last_error(), "win_host"));
  CHECK(smi_pitchs_create(1, 100, 16, 3, win, -1, &h) == SMI_EINVAL && std::strstr(smi_last_error(), "max_taps"));
  CHECK(smi_pitchs_create(1, 100, 16, 3, win, 16384, &h) == SMI_EINVAL && std::strstr(smi_last_error(), "max_taps"));
  float taps[3] = {0};
  CHECK(smi_pitchs_open(nullptr, 0, 1, 1, 3, 2, taps, 3, nullptr) == SMI_EINVAL);
  int32_t one[1] = {0};
  float x[1] = {0};
  CHECK(smi_pitchs_push_rows(nullptr, x, 1, one, one, one, 1, nullptr, 0, x, 1, nullptr, nullptr) == SMI_EINVAL);
  CHECK(smi_pitchs_destroy(nullptr) == SMI_OK);
  std::printf("pitchs host check ok: %lld streams, %lld pushes\n", streams, pushes);
  return 0;
}
