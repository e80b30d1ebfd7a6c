// Request program (include/gd4d.h): the launch sequence of one eager decoder request, kept on the host side of the library and
// re-issued by one call.  Host code only - this translation unit holds no kernel; every step calls an entry point of the library
// (or hipEventRecord / hipStreamWaitEvent / hipMemcpyAsync) with the arguments the table holds.
#include <string.h>

#include <new>
#include <vector>

#include "gd4d_common.h"

namespace {

struct Step {
  gd4d_request_step s;                       // the caller's record; its pointers are redirected to the copies below
  std::vector<gd4d_chain_op> prog_a, prog_b;
  gd4d_chain_guest guest;
  std::vector<gd4d_request_patch> patches;
  std::vector<uint64_t> table[GD4D_REQ_TABLES];      // (8-byte units: pointer and int64 arrays stay aligned)
};

bool is_chain(int kind) { return kind == GD4D_REQ_ROW_CHAIN || kind == GD4D_REQ_ROW_CHAIN2 || kind == GD4D_REQ_ROW_CHAIN_GUEST; }

// pointer arguments / tables / integers a kind reads
struct Shape {
  const char* name;
  int ptrs, tables;
};

const Shape* shape_of(int kind) {
  static const Shape shapes[] = {
      {nullptr, 0, 0},
      {"gd4d_row_chain_fwd", 0, 0},
      {"gd4d_row_chain2_fwd", 0, 0},
      {"gd4d_row_chain_guest_fwd", 0, 0},
      {"gd4d_mha_core_fwd", 5, 0},
      {"gd4d_mha_core_presplit_fwd", 5, 0},
      {"gd4d_cross_attn_plan_fwd", 10, 3},
      {"gd4d_cross_attn_agg_items_coarse_fwd", 5, 5},
      {"gd4d_cross_attn_agg_items_fwd", 4, 3},
      {"gd4d_cross_attn_agg_sliced_fwd", 3, 1},
      {"gd4d_pyramid_slice_planar_fwd", 1, 2},
      {"gd4d_value_proj_guest_fwd", 0, 0},
      {"gd4d_query_order_fwd", 2, 1},
      {"hipEventRecord", 0, 0},
      {"hipStreamWaitEvent", 0, 0},
      {"hipMemcpyAsync", 2, 0},
  };
  if (kind < GD4D_REQ_ROW_CHAIN || kind > GD4D_REQ_COPY) return nullptr;
  return &shapes[kind];
}

// bytes table k of a step must at least hold (0: no such table)
int64_t table_need(const gd4d_request_step& s, int k) {
  const int64_t L = s.kind == GD4D_REQ_SLICE_PLANAR ? s.i[2] : s.kind == GD4D_REQ_PLAN ? s.i[4] : s.i[5];
  switch (s.kind) {
    case GD4D_REQ_PLAN: return k == 0 ? 48 : k == 1 ? 8 * L : 8 * L;
    case GD4D_REQ_AGG_COARSE: return k == 0 ? 8 * L : k == 1 ? 8 * L : k == 2 ? 8 * L : 16;
    case GD4D_REQ_AGG_ITEMS: return 8 * L;
    case GD4D_REQ_AGG_SLICED: return 8 * L;
    case GD4D_REQ_SLICE_PLANAR: return 8 * L;
    case GD4D_REQ_QUERY_ORDER: return 48;
  }
  return 0;
}

}  // namespace

struct gd4d_decoder_request {
  std::vector<Step> steps;
  std::vector<hipEvent_t> events;
  hipEvent_t join = nullptr;                 // joins the side stream back after a failed step
  int nbindings = 0;
  bool uses_side = false;
};

namespace {

int validate(const gd4d_request_step* steps, int nsteps, int nbindings) {
  if (steps == nullptr || nsteps <= 0 || nsteps > GD4D_REQ_MAX_STEPS || nbindings < 0) return GD4D_EINVAL;
  bool recorded[GD4D_REQ_MAX_EVENTS] = {};
  for (int n = 0; n < nsteps; ++n) {
    const gd4d_request_step& s = steps[n];
    const Shape* sh = shape_of(s.kind);
    if (sh == nullptr || (s.side != 0 && s.side != 1) || s.npatches < 0 || (s.npatches > 0 && s.patches == nullptr)) return GD4D_EINVAL;
    for (int k = 0; k < sh->ptrs; ++k)
      if (s.p[k].binding >= nbindings) return GD4D_EINVAL;
    if (s.kind == GD4D_REQ_PLAN && (s.fbind[0] >= nbindings || s.fbind[1] >= nbindings)) return GD4D_EINVAL;
    if (is_chain(s.kind)) {
      if (s.prog_a == nullptr || s.nops_a <= 0 || s.nops_a > GD4D_CHAIN_MAX_OPS) return GD4D_EINVAL;
      const bool two = s.kind == GD4D_REQ_ROW_CHAIN2 || (s.kind == GD4D_REQ_ROW_CHAIN_GUEST && s.nops_b != 0);
      if (two && (s.prog_b == nullptr || s.nops_b <= 0 || s.nops_a + s.nops_b > GD4D_CHAIN_MAX_OPS)) return GD4D_EINVAL;
      if (s.i[0] <= 0) return GD4D_EINVAL;
    }
    if ((s.kind == GD4D_REQ_ROW_CHAIN_GUEST || s.kind == GD4D_REQ_VALUE_PROJ_GUEST) && s.guest == nullptr) return GD4D_EINVAL;
    for (int k = 0; k < sh->tables; ++k) {
      const int64_t need = table_need(s, k);
      if (s.table[k] == nullptr || need <= 0 || s.table_bytes[k] < need || s.table_bytes[k] > (1 << 20)) return GD4D_EINVAL;
    }
    if (s.kind == GD4D_REQ_EVENT_RECORD || s.kind == GD4D_REQ_STREAM_WAIT) {
      if (s.event < 0 || s.event >= GD4D_REQ_MAX_EVENTS) return GD4D_EINVAL;
      if (s.kind == GD4D_REQ_EVENT_RECORD) recorded[s.event] = true;
      else if (!recorded[s.event]) return GD4D_EINVAL;
    }
    if (s.kind == GD4D_REQ_COPY && s.l[0] <= 0) return GD4D_EINVAL;
    for (int k = 0; k < s.npatches; ++k) {
      const gd4d_request_patch& pt = s.patches[k];
      int64_t size = -1;
      if (pt.table == 0 && is_chain(s.kind)) size = int64_t(s.nops_a) * sizeof(gd4d_chain_op);
      else if (pt.table == 1 && s.kind != GD4D_REQ_ROW_CHAIN && is_chain(s.kind) && s.prog_b != nullptr && s.nops_b > 0)
        size = int64_t(s.nops_b) * sizeof(gd4d_chain_op);   // (only the kinds that keep a second program)
      else if (pt.table == 2 && s.guest != nullptr) size = sizeof(gd4d_chain_guest);
      else if (pt.table >= 3 && pt.table < 3 + sh->tables) size = s.table_bytes[pt.table - 3];
      if (pt.binding < 0 || pt.binding >= nbindings || pt.offset < 0 || (pt.offset & 7) || pt.offset + 8 > size) return GD4D_EINVAL;
    }
  }
  return GD4D_OK;
}

inline void* at(const gd4d_request_ref& r, const gd4d_request_binding* b) {
  if (r.binding < 0) return reinterpret_cast<void*>(static_cast<uintptr_t>(r.value));
  return const_cast<char*>(static_cast<const char*>(b[r.binding].ptr)) + r.value;
}

int issue(gd4d_decoder_request* req, Step& st, const gd4d_request_binding* b, hipStream_t stream) {
  gd4d_request_step& s = st.s;
  for (const gd4d_request_patch& pt : st.patches) {
    char* base = pt.table == 0 ? reinterpret_cast<char*>(st.prog_a.data())
               : pt.table == 1 ? reinterpret_cast<char*>(st.prog_b.data())
               : pt.table == 2 ? reinterpret_cast<char*>(&st.guest)
                               : reinterpret_cast<char*>(st.table[pt.table - 3].data());
    const char* v = static_cast<const char*>(b[pt.binding].ptr) + pt.add;
    memcpy(base + pt.offset, &v, sizeof(v));
  }
  const int32_t* i = s.i;
  auto P = [&](int k) { return at(s.p[k], b); };
  auto F = [&](int k) { return static_cast<float*>(at(s.p[k], b)); };
  auto T = [&](int k) { return static_cast<const void*>(st.table[k].data()); };
  const gd4d_chain_op* pa = st.prog_a.data();
  const gd4d_chain_op* pb = st.prog_b.empty() ? nullptr : st.prog_b.data();
  switch (s.kind) {
    case GD4D_REQ_ROW_CHAIN: return gd4d_row_chain_fwd(pa, s.nops_a, i[0], stream);
    case GD4D_REQ_ROW_CHAIN2: return gd4d_row_chain2_fwd(pa, s.nops_a, pb, s.nops_b, i[0], stream);
    case GD4D_REQ_ROW_CHAIN_GUEST: return gd4d_row_chain_guest_fwd(pa, s.nops_a, pb, s.nops_b, i[0], &st.guest, stream);
    case GD4D_REQ_MHA_CORE:
      return gd4d_mha_core_fwd(F(0), F(1), F(2), P(3), F(4), i[0], i[1], i[2], i[3], i[4], i[5], i[6], i[7], i[8], i[9], s.f[0], nullptr,
                               0.f, nullptr, stream);
    case GD4D_REQ_MHA_PRESPLIT:
      return gd4d_mha_core_presplit_fwd(F(0), P(1), P(2), F(3), i[0], i[1], i[2], i[3], i[4], s.l[0], s.l[1], P(4), i[5], s.f[0], nullptr,
                                        0.f, nullptr, stream);
    case GD4D_REQ_PLAN: {
      const float img_h = s.fbind[0] >= 0 ? static_cast<float>(b[s.fbind[0]].scalar) : s.f[0];
      const float img_w = s.fbind[1] >= 0 ? static_cast<float>(b[s.fbind[1]].scalar) : s.f[1];
      return gd4d_cross_attn_plan_fwd(F(0), F(1), F(2), F(3), F(4), static_cast<const double*>(T(0)), img_h, img_w,
                                      static_cast<const int32_t*>(T(1)), static_cast<const int64_t*>(T(2)), s.l[0], P(5),
                                      static_cast<size_t>(s.l[1]), F(6), static_cast<uint8_t*>(P(7)), F(8), i[0], i[1], i[2], i[3], i[4],
                                      i[5], i[6], static_cast<const int32_t*>(P(9)), stream);
    }
    case GD4D_REQ_AGG_COARSE:
      return gd4d_cross_attn_agg_items_coarse_fwd(static_cast<const void* const*>(T(0)), static_cast<const int32_t*>(T(1)),
                                                  static_cast<const int64_t*>(T(2)), s.l[0], s.l[1], static_cast<const void* const*>(T(3)),
                                                  static_cast<const int64_t*>(T(4)), P(0), F(1), F(2), F(3), i[0], i[1], i[2], i[3], i[4],
                                                  i[5], i[6], i[7], static_cast<const int32_t*>(P(4)), stream);
    case GD4D_REQ_AGG_ITEMS:
      return gd4d_cross_attn_agg_items_fwd(static_cast<const void* const*>(T(0)), static_cast<const int32_t*>(T(1)),
                                           static_cast<const int64_t*>(T(2)), s.l[0], s.l[1], P(0), F(1), F(2), i[0], i[1], i[2], i[3], i[4],
                                           i[5], i[6], i[7], static_cast<const int32_t*>(P(3)), i[8], i[9], stream);
    case GD4D_REQ_AGG_SLICED:
      return gd4d_cross_attn_agg_sliced_fwd(static_cast<const void* const*>(T(0)), s.l[0], P(0), F(1), i[0], i[1], i[2], i[3], i[4], i[5],
                                            i[6], i[7], static_cast<const int32_t*>(P(2)), i[8], i[9], stream);
    case GD4D_REQ_SLICE_PLANAR:
      return gd4d_pyramid_slice_planar_fwd(static_cast<const void* const*>(T(0)), static_cast<const int32_t*>(T(1)), P(0), i[0], i[1], i[2],
                                           i[3], i[4], i[5], stream);
    case GD4D_REQ_VALUE_PROJ_GUEST: return gd4d_value_proj_guest_fwd(&st.guest, i[0], stream);
    case GD4D_REQ_QUERY_ORDER:
      return gd4d_query_order_fwd(F(0), static_cast<const double*>(T(0)), static_cast<int32_t*>(P(1)), i[0], i[1], stream);
    case GD4D_REQ_EVENT_RECORD:
    case GD4D_REQ_STREAM_WAIT:
    case GD4D_REQ_COPY: {
      hipError_t e = s.kind == GD4D_REQ_EVENT_RECORD  ? hipEventRecord(req->events[s.event], stream)
                     : s.kind == GD4D_REQ_STREAM_WAIT ? hipStreamWaitEvent(stream, req->events[s.event], 0)
                                                      : hipMemcpyAsync(P(0), P(1), static_cast<size_t>(s.l[0]), hipMemcpyDeviceToDevice, stream);
      if (e != hipSuccess) {
        gd4d::set_last_hip_error(e);
        return GD4D_ELAUNCH;
      }
      return GD4D_OK;
    }
  }
  return GD4D_EINVAL;
}

void release(gd4d_decoder_request* req) {
  for (hipEvent_t e : req->events)
    if (e != nullptr) (void)hipEventDestroy(e);
  if (req->join != nullptr) (void)hipEventDestroy(req->join);
  delete req;
}

}  // namespace

extern "C" size_t gd4d_request_step_bytes(void) { return sizeof(gd4d_request_step); }

extern "C" int gd4d_decoder_request_create(const gd4d_request_step* steps, int nsteps, int nbindings, gd4d_decoder_request** out) {
  if (out == nullptr) return GD4D_EINVAL;
  *out = nullptr;
  const int code = validate(steps, nsteps, nbindings);
  if (code != GD4D_OK) return code;
  gd4d_decoder_request* req = new (std::nothrow) gd4d_decoder_request();
  if (req == nullptr) return GD4D_EINVAL;
  req->nbindings = nbindings;
  req->steps.resize(nsteps);
  int nevents = 0;
  for (int n = 0; n < nsteps; ++n) {
    Step& st = req->steps[n];
    st.s = steps[n];
    gd4d_request_step& s = st.s;
    const Shape* sh = shape_of(s.kind);
    memset(&st.guest, 0, sizeof(st.guest));
    if (is_chain(s.kind)) {
      st.prog_a.assign(s.prog_a, s.prog_a + s.nops_a);
      if (s.prog_b != nullptr && s.nops_b > 0 && s.kind != GD4D_REQ_ROW_CHAIN) st.prog_b.assign(s.prog_b, s.prog_b + s.nops_b);
      else s.nops_b = 0;
    }
    if (s.guest != nullptr && (s.kind == GD4D_REQ_ROW_CHAIN_GUEST || s.kind == GD4D_REQ_VALUE_PROJ_GUEST)) st.guest = *s.guest;
    if (s.npatches > 0) st.patches.assign(s.patches, s.patches + s.npatches);
    for (int k = 0; k < sh->tables; ++k) {
      st.table[k].assign(static_cast<size_t>((s.table_bytes[k] + 7) / 8), 0);
      memcpy(st.table[k].data(), s.table[k], static_cast<size_t>(s.table_bytes[k]));
    }
    // the copies are what run() reads: nothing of the caller's memory is referred to after this call
    s.prog_a = s.prog_b = nullptr;
    s.guest = nullptr;
    s.patches = nullptr;
    for (int k = 0; k < GD4D_REQ_TABLES; ++k) s.table[k] = nullptr;
    if (s.kind == GD4D_REQ_EVENT_RECORD && s.event + 1 > nevents) nevents = s.event + 1;
    if (s.side != 0) req->uses_side = true;
  }
  req->events.assign(nevents, nullptr);
  for (int n = 0; n < nevents + (req->uses_side ? 1 : 0); ++n) {
    hipEvent_t e = nullptr;
    hipError_t err = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (err != hipSuccess) {
      gd4d::set_last_hip_error(err);
      release(req);
      return GD4D_ELAUNCH;
    }
    if (n < nevents) req->events[n] = e;
    else req->join = e;
  }
  *out = req;
  return GD4D_OK;
}

extern "C" int gd4d_decoder_request_run(gd4d_decoder_request* req, const gd4d_request_binding* bindings, int nbindings, void* stream,
                                        void* side_stream) {
  if (req == nullptr || nbindings != req->nbindings || (nbindings > 0 && bindings == nullptr)) return GD4D_EINVAL;
  if (req->uses_side && (side_stream == nullptr || side_stream == stream)) return GD4D_EINVAL;
  hipStream_t main_s = static_cast<hipStream_t>(stream), side_s = static_cast<hipStream_t>(side_stream);
  bool side_touched = false;
  for (Step& st : req->steps) {
    const bool side = st.s.side != 0;
    const int code = issue(req, st, bindings, side ? side_s : main_s);
    if (code != GD4D_OK) {
      // whatever the side stream was given so far ends in `stream`: the caller's stream holds no wait for an event nobody records, and
      // the side stream has no work the caller cannot order against
      if (side_touched && hipEventRecord(req->join, side_s) == hipSuccess) (void)hipStreamWaitEvent(main_s, req->join, 0);
      return code;
    }
    side_touched = side_touched || side;
  }
  return GD4D_OK;
}

extern "C" int gd4d_decoder_request_destroy(gd4d_decoder_request* req) {
  if (req == nullptr) return GD4D_EINVAL;
  release(req);
  return GD4D_OK;
}

extern "C" const char* gd4d_decoder_request_describe(const gd4d_decoder_request* req, int i) {
  if (req == nullptr || i < 0 || i >= static_cast<int>(req->steps.size())) return nullptr;
  return shape_of(req->steps[i].s.kind)->name;
}
