// Stand-alone host check of the launch helpers of skrample_amd/csrc/skr_launch.h and of the step dtype rule (skr_step_common.h), for a
// sanitizer build that runs on the CPU (no device is touched, nothing is loaded into Python):
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/launch_helpers_check.hip -o /tmp/launch_helpers_check && /tmp/launch_helpers_check
//
// Walks every dtype code from -2 to 5 through both families of with_dtype with a counting functor, every flag combination through
// with_bools, check_ptrs over arrays with a missing / misaligned entry at every position (and n = 0 with no array), grid_blocks at its
// edges, and the dtype rule against the nine (group a, group b, arithmetic) triples the step kernels exist for.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../skrample_amd/csrc/skr_step_common.h"

namespace skr { Tuning g_tune; }  // (skr_step_common.h declares it; defined by skr_step.hip in the library)

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

template <typename Family, bool WITH_F64>
static void walk_dtypes() {
  for (int32_t code = -2; code <= 5; ++code) {
    int calls = 0;
    size_t size = 0;
    const int rc = skr::with_dtype<Family, WITH_F64>(code, [&](auto t) { ++calls; size = sizeof(typename decltype(t)::type); return 40 + code; });
    const bool valid = code == SKR_BF16 || code == SKR_F16 || code == SKR_F32 || (WITH_F64 && code == SKR_F64);
    CHECK(calls == (valid ? 1 : 0));
    CHECK(rc == (valid ? 40 + code : (int)SKR_ERR_DTYPE));
    if (valid) CHECK(size == (code == SKR_F64 ? 8u : (code == SKR_F32 ? 4u : 2u)));
    calls = 0;
    const int rv = skr::with_dtype<Family, WITH_F64>(code, [&](auto) { ++calls; });  // a launcher that returns nothing
    CHECK(calls == (valid ? 1 : 0) && rv == (valid ? (int)SKR_OK : (int)SKR_ERR_DTYPE));
  }
}

int main() {
  walk_dtypes<skr::NoiseTypes, true>();
  walk_dtypes<skr::NoiseTypes, false>();
  walk_dtypes<skr::StepTypes, true>();
  walk_dtypes<skr::StepTypes, false>();
  CHECK(skr::with_step_type(SKR_BF16, [](auto t) { return (int)std::is_same<typename decltype(t)::type, skr::bf16_t>::value; }) == 1);
  CHECK(skr::with_out_type(SKR_F16, [](auto t) { return (int)std::is_same<typename decltype(t)::type, _Float16>::value; }) == 1);

  for (int bits = 0; bits < 8; ++bits) {
    int calls = 0;
    const int got = skr::with_bools([&](auto a, auto b, auto c) { ++calls; return (a ? 1 : 0) | (b ? 2 : 0) | (c ? 4 : 0); }, (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0);
    CHECK(got == bits && calls == 1);
  }

  CHECK(skr::check_ptrs(nullptr, 0) == SKR_OK);
  alignas(16) static char storage[16 * 8];
  for (int n = 1; n <= 7; ++n) {
    std::vector<const void*> p(n);  // (exactly n entries: a read past the count is a heap overflow the sanitizer reports)
    for (int k = 0; k < n; ++k) p[k] = storage + 16 * k;
    CHECK(skr::check_ptrs(p.data(), n) == SKR_OK);
    for (int k = 0; k < n; ++k) {
      std::vector<const void*> q(p);
      q[k] = nullptr;
      CHECK(skr::check_ptrs(q.data(), n) == SKR_ERR_NULL);
      CHECK(skr::check_ptrs(q.data(), k) == SKR_OK);  // (the fault lies beyond the count)
      q[k] = storage + 16 * k + 2;
      CHECK(skr::check_ptrs(q.data(), n) == SKR_ERR_ALIGN);
      if (k + 1 < n) {  // the first fault decides
        q[k + 1] = nullptr;
        CHECK(skr::check_ptrs(q.data(), n) == SKR_ERR_ALIGN);
        q[k] = nullptr;
        q[k + 1] = storage + 1;
        CHECK(skr::check_ptrs(q.data(), n) == SKR_ERR_NULL);
      }
    }
  }
  CHECK(skr::aligned16(storage) && !skr::aligned16(storage + 8) && skr::aligned16(nullptr));

  CHECK(skr::grid_blocks(0, 256, 1024) == 0 && skr::grid_blocks(1, 256, 1024) == 1 && skr::grid_blocks(256, 256, 1024) == 1 && skr::grid_blocks(257, 256, 1024) == 2);
  CHECK(skr::grid_blocks(256ll * 1024, 256, 1024) == 1024 && skr::grid_blocks(256ll * 1024 + 1, 256, 1024) == 1024 && skr::grid_blocks((int64_t)1 << 62, 256, 256 * 64) == 256 * 64);

  int admitted = 0;
  for (int acc = 0; acc < 2; ++acc)
    for (int32_t da = -2; da <= 5; ++da)
      for (int32_t db = -2; db <= 5; ++db) {
        const bool a16 = da == SKR_BF16 || da == SKR_F16;
        const bool want = acc ? ((da == SKR_F64 && db == SKR_F64) || ((a16 || da == SKR_F32) && (db == da || db == SKR_F64)))
                              : ((a16 && (db == da || db == SKR_F32)) || (da == SKR_F32 && db == SKR_F32));
        CHECK(skr::step_inputs_ok(da, db, acc != 0) == want);
        admitted += want;
        if (want) for (int32_t o = -2; o <= 5; ++o) CHECK(skr::step_output_ok(o, da, acc != 0) == (o == da || o == (acc ? SKR_F64 : SKR_F32)));
      }
  CHECK(admitted == 5 + 7);  // fp32 arithmetic: 5 pairs; fp64: 7 pairs of codes, which share the 4 kernels that read group b as fp64
  std::puts("launch helpers: ok");
  return 0;
}
