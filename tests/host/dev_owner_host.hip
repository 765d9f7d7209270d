// Stand-alone check of DevBuf (spark-tts_amd/csrc/smi_common.h), the owner of every device allocation of libsparkmi.
// tests/test_dev_owner_cpu.py builds it with the host half under AddressSanitizer / UBSan and runs it on a machine without a
// GPU, where every hipMalloc fails at once: that failure is the path under test.  (With a GPU the same checks take the
// successful branches; the pytest never runs the instrumented build there.)
#include "smi_common.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <utility>

std::atomic<long long> g_smi_dev_live{0}, g_smi_dev_bytes{0};
static char g_err[512] = "";
void smi_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

static int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++g_failed; } } while (0)

static bool counters(long long live, long long bytes) { return g_smi_dev_live.load() == live && g_smi_dev_bytes.load() == bytes; }

template <bool PINNED>
static void exercise() {
  const size_t n = 4096, big = (size_t)1 << 20;
  CHECK(counters(0, 0));
  {
    DevBuf<float, PINNED> a;
    CHECK(!a && a.get() == nullptr && a.bytes() == 0);
    a.reset();   // reset of an empty owner: nothing happens
    CHECK(!a && counters(0, 0));
    g_err[0] = 0;
    const int rc = a.alloc(n, "probe");
    if (rc != SMI_OK) {   // no device: the owner stays empty, the counters stay, the text names the buffer and the byte count
      CHECK(rc == SMI_ENOMEM && !a && a.bytes() == 0 && counters(0, 0));
      CHECK(strstr(g_err, "probe") && strstr(g_err, "4096 bytes") && strstr(g_err, PINNED ? "hipHostMalloc" : "hipMalloc"));
      CHECK(a.alloc_zero(n, "probe") == SMI_ENOMEM && !a && counters(0, 0));
      CHECK(a.ensure(n, "probe") == SMI_ENOMEM && !a && a.bytes() == 0);
      CHECK(a.ensure(big, "probe") == SMI_ENOMEM && !a && a.bytes() == 0 && counters(0, 0));   // ensure after a failed ensure: still empty
    } else {
      CHECK(a && a.bytes() == n && counters(1, (long long)n));
      float* const p = a;
      CHECK(a.ensure(n / 2, "probe") == SMI_OK && (float*)a == p && a.bytes() == n);   // large enough: the same allocation
      CHECK(a.ensure(big, "probe") == SMI_OK && a.bytes() == big && counters(1, (long long)big));
      CHECK(a.alloc_zero(n, "probe") == SMI_OK && a.bytes() == n && counters(1, (long long)n));
    }
    const bool held = a;
    const size_t held_bytes = a.bytes();
    DevBuf<float, PINNED> b(std::move(a));   // move-construct: the source is empty, the allocation counted once
    CHECK(!a && a.bytes() == 0 && (bool)b == held && b.bytes() == held_bytes && counters(held ? 1 : 0, (long long)held_bytes));
    DevBuf<float, PINNED> c;
    c = std::move(b);                        // move-assign
    CHECK(!b && b.bytes() == 0 && (bool)c == held && c.bytes() == held_bytes && counters(held ? 1 : 0, (long long)held_bytes));
    c = std::move(c);                        // onto itself: unchanged
    CHECK((bool)c == held && c.bytes() == held_bytes);
    DevBuf<float, PINNED> d;
    c = std::move(d);                        // an empty one moved in: what c held is freed
    CHECK(!c && !d && counters(0, 0));
  }   // destructors of empty owners: nothing happens
  CHECK(counters(0, 0));
  {
    DevBuf<void> v;   // (the KV cache's element type is chosen at run time)
    (void)v.alloc(n, "void probe");
  }                   // whatever it got goes with the scope
  CHECK(counters(0, 0));
}

int main() {
  exercise<false>();
  exercise<true>();
  if (g_failed) { fprintf(stderr, "dev_owner_host: %d checks failed\n", g_failed); return 1; }
  printf("dev_owner_host ok\n");
  return 0;
}
