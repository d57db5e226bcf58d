// Stand-alone host check of the launch helpers of skrample_amd/csrc/skr_launch.h and of the step dtype rule (skr_step_common.h), for a
// sanitizer build that runs on the CPU (no device is touched, nothing is loaded into Python):
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/launch_helpers_check.hip -o /tmp/launch_helpers_check && /tmp/launch_helpers_check
//
// Walks every dtype code from -2 to 5 through both families of with_dtype with a counting functor, every flag combination through
// with_bools, check_ptrs over arrays with a missing / misaligned entry at every position (and n = 0 with no array), grid_blocks at its
// edges, the dtype rule against the nine (group a, group b, arithmetic) triples the step kernels exist for, and choose_pyramid_route over
// a table of edge shapes, each with its neighbour across the threshold (the values: an exhaustive comparison with the decision this
// function replaced, every h <= 1024, every w <= 1024, both switches).
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

// (h, w, resize_h, SKR_PYR_NO_UNI, SKR_PYR_MODE) -> status, form, threads, dynamic LDS bytes, offset of the tap table
struct RouteRow { int64_t h, w; bool resize_h, no_uni; int forced; int status; skr::PyramidForm form; int threads; size_t lds_bytes; int32_t ytab_off; };
using F = skr::PyramidForm;
static const RouteRow ROUTES[] = {
    // small planes: generic
    {16, 16, true, false, 0, SKR_OK, F::Generic, 512, 528, -1},
    // one resized axis: generic at every width
    {1, 64, false, false, 0, SKR_OK, F::Generic, 512, 424, -1},
    {1, 1024, false, false, 0, SKR_OK, F::Generic, 512, 2944, -1},
    // w / 4 divides no block size: generic, 16043 floats of levels, LDS opt-in
    {200, 300, true, false, 0, SKR_OK, F::Generic, 512, 64172, -1},
    // 12 rows per 256-lane strip
    {95, 128, true, false, 0, SKR_OK, F::Generic, 512, 13024, -1},
    {96, 128, true, false, 0, SKR_OK, F::Strip256, 256, 13360, -1},
    // 12 rows per 512-lane strip
    {191, 128, true, false, 0, SKR_OK, F::Strip256, 256, 26128, -1},
    {192, 128, true, false, 0, SKR_OK, F::Strip512, 512, 26464, -1},
    // 12 rows per 1024-lane strip; rows of half a wave: no UNI (52 672 B, opt-in)
    {383, 128, true, false, 0, SKR_OK, F::Strip512, 512, 52336, -1},
    {384, 128, true, false, 0, SKR_OK, F::Strip1024, 1024, 52672, -1},
    // UNI: rows a whole number of waves wide and 12 rows per 1024-lane strip
    {191, 256, true, false, 0, SKR_OK, F::Strip512, 512, 52000, -1},
    {192, 256, true, false, 0, SKR_OK, F::Uni, 1024, 58816, 13168},
    {95, 512, true, false, 0, SKR_OK, F::Strip512, 512, 51328, -1},
    {96, 512, true, false, 0, SKR_OK, F::Uni, 1024, 55744, 13168},
    {47, 1024, true, false, 0, SKR_OK, F::Strip512, 512, 50048, -1},
    {48, 1024, true, false, 0, SKR_OK, F::Uni, 1024, 54144, 13152},
    // the cfg5 plane
    {256, 256, true, false, 0, SKR_OK, F::Uni, 1024, 78336, 17536},
    // rows of 256 lanes: one row per 256-lane strip
    {11, 1024, true, false, 0, SKR_OK, F::Generic, 512, 11008, -1},
    {12, 1024, true, false, 0, SKR_OK, F::Strip256, 256, 13056, -1},
    // the tap table must fit 156 KiB behind the levels
    {523, 256, true, false, 0, SKR_OK, F::Uni, 1024, 159456, 35680},
    {524, 256, true, false, 0, SKR_OK, F::Strip1024, 1024, 143232, -1},
    // the level stage holds 38 * 1024 floats
    {383, 380, true, false, 0, SKR_OK, F::Generic, 512, 154736, -1},
    {384, 380, true, false, 0, SKR_ERR_UNSUPPORTED, F::Generic, 0, 0, -1},
    // (bound 42 708)
    {400, 400, true, false, 0, SKR_ERR_UNSUPPORTED, F::Generic, 0, 0, -1},
    // (30, 90) with a width the entry point takes
    {30, 92, true, false, 0, SKR_OK, F::Generic, 512, 3148, -1},
    // SKR_PYR_NO_UNI
    {256, 256, true, true, 0, SKR_OK, F::Strip1024, 1024, 70144, -1},
    {96, 512, true, true, 0, SKR_OK, F::Strip1024, 1024, 52672, -1},
    // forced forms: the tap table stays laid out under a forced generic form
    {256, 256, true, false, 1, SKR_OK, F::Generic, 512, 78336, 17536},
    {256, 256, true, false, 2, SKR_OK, F::Strip512, 512, 78336, 17536},
    // strip / 256 refuses more than 48 KiB: generic
    {256, 256, true, false, 3, SKR_OK, F::Generic, 512, 78336, 17536},
    {256, 256, true, false, 4, SKR_OK, F::Uni, 1024, 78336, 17536},
    {96, 128, true, false, 1, SKR_OK, F::Generic, 512, 13360, -1},
    // a forced form whose run is too short: generic
    {96, 128, true, false, 2, SKR_OK, F::Generic, 512, 13360, -1},
    {96, 128, true, false, 3, SKR_OK, F::Strip256, 256, 13360, -1},
    {96, 128, true, false, 4, SKR_OK, F::Generic, 512, 13360, -1},
    // forcing a smaller block than the shape would get
    {192, 128, true, false, 3, SKR_OK, F::Strip256, 256, 26464, -1},
    {384, 128, true, false, 2, SKR_OK, F::Strip512, 512, 52672, -1},
    // (52 672 B)
    {384, 128, true, false, 3, SKR_OK, F::Generic, 512, 52672, -1},
    {16, 16, true, false, 4, SKR_OK, F::Generic, 512, 528, -1},
    // no such mode: generic
    {192, 128, true, false, 7, SKR_OK, F::Generic, 512, 26464, -1},
};

static void walk_pyramid_routes() {
  for (const RouteRow& x : ROUTES) {
    const skr::PyramidRoute r = skr::choose_pyramid_route(x.h, x.w, x.resize_h, x.no_uni, x.forced);
    const bool same = r.status == x.status && (r.status != SKR_OK || (r.form == x.form && r.threads == x.threads && r.lds_bytes == x.lds_bytes && r.ytab_off == x.ytab_off));
    if (!same) std::fprintf(stderr, "route of (%ld, %ld, %d, %d, %d): status %d form %d threads %d lds %zu ytab %d\n", (long)x.h, (long)x.w, (int)x.resize_h, (int)x.no_uni, x.forced,
                            r.status, (int)r.form, r.threads, r.lds_bytes, (int)r.ytab_off);
    CHECK(same);
  }
}

int main() {
  walk_pyramid_routes();
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
