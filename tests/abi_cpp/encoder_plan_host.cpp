// The host plan of an encoder forward and the knob table (gmf_amd/csrc/encoder_plan.hpp) on their own: built by the host compiler
// with -fsanitize=address,undefined (tests/test_encoder_plan_host.py).
//  1. One line per plan with every EncoderPlan field, over shapes x {default knobs, every knob moved alone, every optional weight
//     image missing alone, the dense drop-in}: the test compares them with tests/golden/encoder_plan_table.txt, which was printed
//     by the plan as it stood before it moved into the header.  The knobs are moved through the struct's fields, not through the
//     knob table, so the lines do not depend on part 3.
//  2. Invariants of every such plan, written out here independently of the plan code.
//  3. The knob table: names, accepted values, defaults and errors, against the values written out below.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../gmf_amd/csrc/encoder_plan.hpp"

#define CHECK(c)                                                                           \
  do {                                                                                     \
    if (!(c)) {                                                                            \
      std::printf("encoder_plan_host: %s failed (line %d) at %s\n", #c, __LINE__, g_where.c_str()); \
      return 1;                                                                            \
    }                                                                                      \
  } while (0)

static std::string g_where = "start";

// ---- 1. the table ------------------------------------------------------------------------------------------------------------------
static float g_blob[4];   // what every weight pointer points at: the plan asks only whether an image is there

static gmf_encoder_weights all_weights(int L) {
  gmf_encoder_weights w;
  std::memset(&w, 0, sizeof w);
  w.num_layers = L;
  w.sigma_d = 0.1f;
  const float* p = g_blob;
  w.f1_ctx_wst = w.f1_ctx_vec = w.f1_attn_wst = w.f1_attn_vec = w.f1_ff_wst = w.f1_ff_vec = p;
  w.ctx_wst = w.ctx_vec = w.attn_wst = w.attn_vec = w.ff_wst = w.ff_vec = w.front_wst = w.front_vec = w.tail_wst = w.tail_vec = p;
  w.head_wst = w.head_vec = p;
  w.front_wst_h2 = w.ctx_wst_h2 = w.attn_wst_h2 = w.ff_wst_h2 = w.f1_ctx_wst_h2 = w.f1_attn_wst_h2 = w.f1_ff_wst_h2 = w.tail_wst_h2 = p;
  w.pv_guard = w.kv_fold = p;
  return w;
}

struct Shape { int B, N, L, min_tiles; const char* ragged; };

constexpr int kCus = 256, kT = 196;

static int check_invariants(const EncoderPlan& p, const Shape& s) {
  const int tiles = (s.N + 31) / 32;
  const int W = ((tiles + 3) / 4) * s.B;
  if (p.c16_guard) CHECK(p.fmt == 2 && p.form == EncoderPlan::kLinear && p.guard && p.cache_fb_floats > 0);
  if (p.kv_fold) CHECK(p.form == EncoderPlan::kLinear && p.pipelined && !p.half);
  if (p.q_in_attn) CHECK(p.form == EncoderPlan::kLinear && !p.roles && !p.half);
  if (p.prologue) CHECK(p.fmt == 0 && p.fused());
  if (p.form == EncoderPlan::kSmall3) CHECK(p.attn_nf == 0 && p.attn_ks > 1 && p.ff_hs > 1 && p.max_splits == 8);
  CHECK(p.attn_ks <= (p.max_splits > 1 ? p.max_splits : 1));
  CHECK(p.ff_hs == 1 || p.ff_hs == 2 || p.ff_hs == 4 || p.ff_hs == 8);
  CHECK((p.cache_floats + p.cache_fb_floats) * 4 <= ((size_t)96 << 30));
  if (s.min_tiles > 0) CHECK(p.attn_nf == 0 || p.attn_nf == (W + 7) / 8);   // ragged: every item split, or none
  return 0;
}

// One line per plan, "<what>=<value> : <fields>", under the line that names its shape.  The shape's first line, the plan under the
// default knobs, ends with act and tok; they depend on the shape alone, which every other plan of the shape is checked for here
// instead of printing them again.  A plan equal to that first one in every field prints "=" for its fields.
static std::string g_default_fields;
static size_t g_default_act, g_default_tok;

static int row(const Shape& s, const char* what, int value, const gmf::Tuning& t, const gmf_encoder_weights& w, bool dense) {
  char label[96], fields[160];
  std::snprintf(label, sizeof label, "%s=%d", what, value);
  g_where = std::to_string(s.B) + "x" + std::to_string(s.N) + " L" + std::to_string(s.L) + " " + s.ragged + " " + label;
  const EncoderPlan p = plan_encoder(t, &w, s.B, s.N, kT, s.L, s.min_tiles, kCus, dense);
  std::snprintf(fields, sizeof fields, "%d %d%d%d%d%d%d%d%d%d%d%d%d%d%d %d %d %d %d %d %d %zu %zu", (int)p.form, (int)p.f1_h2,
                (int)p.prologue, (int)p.cache, (int)p.pipelined, (int)p.half, (int)p.one_product, (int)p.front_split, (int)p.roles,
                (int)p.q_in_attn, (int)p.kv_fold, (int)p.c16_guard, (int)p.v_fp8, (int)p.guard, (int)p.clear_stats, p.fmt, p.max_splits,
                p.attn_nf, p.attn_ks, p.ff_hs, p.f1_ff_hs, p.cache_floats, p.cache_fb_floats);
  if (std::strcmp(what, "default") == 0) {
    g_default_fields = fields;
    g_default_act = p.act;
    g_default_tok = p.tok;
    std::printf("%s : %s %zu %zu\n", label, fields, p.act, p.tok);
  } else {
    CHECK(p.act == g_default_act && p.tok == g_default_tok);
    std::printf("%s : %s\n", label, g_default_fields == fields ? "=" : fields);
  }
  return check_invariants(p, s);
}

// a knob of struct Tuning and the accepted values other than its default (range knobs: their ends and 1)
struct IntMove { const char* name; int gmf::Tuning::*field; std::vector<int> others; };
struct BoolMove { const char* name; bool gmf::Tuning::*field; };

static int table() {
  using T = gmf::Tuning;
  const std::vector<IntMove> ints = {
      {"scattn_variant", &T::scattn_variant, {0, 9}},  {"ff_hidden_splits", &T::ff_split, {1, 2, 4, 8}},
      {"attn_key_splits", &T::key_splits, {1, 8}},     {"conv_lds_patch", &T::conv_patch, {0, 2}},
      {"nms_binned", &T::nms_binned, {0, 2}},          {"mid_grid_roles", &T::mid_grid_roles, {0, 1, 4096}},
      {"pv_fp8", &T::pv_fp8, {0, 2}},                  {"compat_format", &T::compat_format, {2}},
      {"compat_16", &T::compat_16, {0, 2}},            {"precision", &T::precision, {1, 2}},
      {"spectral_col_splits", &T::spectral_col_splits, {1, 32}}, {"clique_local_rows", &T::clique_local_rows, {0, 1}}};
  const std::vector<BoolMove> bools = {
      {"front_output_split", &T::front_split},   {"attn_tail_split", &T::tail_split},         {"small_grid_roles", &T::small_roles},
      {"fused_linear", &T::fused_linear},        {"compat_cache", &T::use_cache},             {"small_fattn_tile", &T::small_fattn_tile},
      {"small_prologue_roles", &T::small_prologue}, {"conv_small_grid", &T::conv_small},      {"topk_select", &T::topk_select},
      {"wide_attn_tile", &T::wide_attn_tile},    {"small_merge_tile", &T::small_merge_tile},  {"q_in_attention", &T::q_in_attention},
      {"kv_fold", &T::kv_fold}};
  struct Missing { const char* name; const float* gmf_encoder_weights::*field; };
  const std::vector<Missing> missing = {
      {"front_wst_h2", &gmf_encoder_weights::front_wst_h2},   {"ctx_wst_h2", &gmf_encoder_weights::ctx_wst_h2},
      {"attn_wst_h2", &gmf_encoder_weights::attn_wst_h2},     {"ff_wst_h2", &gmf_encoder_weights::ff_wst_h2},
      {"tail_wst_h2", &gmf_encoder_weights::tail_wst_h2},     {"f1_ctx_wst_h2", &gmf_encoder_weights::f1_ctx_wst_h2},
      {"f1_attn_wst_h2", &gmf_encoder_weights::f1_attn_wst_h2}, {"f1_ff_wst_h2", &gmf_encoder_weights::f1_ff_wst_h2},
      {"pv_guard", &gmf_encoder_weights::pv_guard},           {"kv_fold", &gmf_encoder_weights::kv_fold}};
  const int BN[][2] = {{1, 256}, {1, 1000}, {1, 5000}, {1, 10000}, {4, 1000}, {8, 2000}, {32, 1000}, {32, 5000}, {40, 5000}};
  const int Ls[] = {1, 2, 12};
  for (const auto& bn : BN) {
    for (int L : Ls) {
      const int tiles = (bn[1] + 31) / 32;
      const Shape shapes[] = {{bn[0], bn[1], L, 0, "uniform"}, {bn[0], bn[1], L, 8, "ragged8"}, {bn[0], bn[1], L, tiles, "raggedN"}};
      for (const Shape& s : shapes) {
        const gmf_encoder_weights w = all_weights(L);
        std::printf("[%dx%d L%d %s]\n", s.B, s.N, s.L, s.ragged);
        if (row(s, "default", 0, T{}, w, false)) return 1;
        for (const IntMove& k : ints)
          for (int v : k.others) {
            T t;
            t.*(k.field) = v;
            if (row(s, k.name, v, t, w, false)) return 1;
          }
        for (const BoolMove& k : bools) {
          T t;
          t.*(k.field) = !(t.*(k.field));
          if (row(s, k.name, t.*(k.field) ? 1 : 0, t, w, false)) return 1;
        }
        for (const Missing& m : missing) {
          gmf_encoder_weights wm = w;
          wm.*(m.field) = nullptr;
          if (row(s, (std::string("no_") + m.name).c_str(), 0, T{}, wm, false)) return 1;
        }
        if (row(s, "dense", 1, T{}, w, true)) return 1;
      }
    }
  }
  return 0;
}

// ---- 3. the knob table -------------------------------------------------------------------------------------------------------------
// Every knob of gmf_set_tuning as the entry point stood before the table: its default, the values it accepted (lo..hi, or the
// listed ones when lo > hi) and some it refused - one below, one above and, for the sets, the gaps.
struct KnobWant { const char* name; int def, lo, hi; std::vector<int> only, refused; };

static int knobs() {
  const std::vector<KnobWant> want = {
      {"scattn_variant", 18, 1, 0, {0, 9, 18}, {-1, 19, 1, 8, 10, 17}},
      {"front_output_split", 1, 0, 1, {}, {-1, 2}},
      {"ff_hidden_splits", 0, 1, 0, {0, 1, 2, 4, 8}, {-1, 9, 3, 5, 6, 7, 16}},
      {"attn_key_splits", 0, 0, 8, {}, {-1, 9}},
      {"attn_tail_split", 0, 0, 1, {}, {-1, 2}},
      {"small_grid_roles", 1, 0, 1, {}, {-1, 2}},
      {"fused_linear", 1, 0, 1, {}, {-1, 2}},
      {"compat_cache", 1, 0, 1, {}, {-1, 2}},
      {"conv_lds_patch", 1, 0, 2, {}, {-1, 3}},
      {"small_fattn_tile", 1, 0, 1, {}, {-1, 2}},
      {"small_prologue_roles", 1, 0, 1, {}, {-1, 2}},
      {"conv_small_grid", 1, 0, 1, {}, {-1, 2}},
      {"nms_binned", 1, 0, 2, {}, {-1, 3}},
      {"topk_select", 1, 0, 1, {}, {-1, 2}},
      {"wide_attn_tile", 1, 0, 1, {}, {-1, 2}},
      {"small_merge_tile", 1, 0, 1, {}, {-1, 2}},
      {"mid_grid_roles", 512, 0, 4096, {}, {-1, 4097}},
      {"q_in_attention", 1, 0, 1, {}, {-1, 2}},
      {"kv_fold", 1, 0, 1, {}, {-1, 2}},
      {"pv_fp8", 1, 0, 2, {}, {-1, 3}},
      {"compat_format", 0, 1, 0, {0, 2}, {-1, 3, 1}},
      {"compat_16", 1, 0, 2, {}, {-1, 3}},
      {"precision", 0, 0, 2, {}, {-1, 3}},
      {"spectral_col_splits", 0, 0, 32, {}, {-1, 33}},
      {"clique_local_rows", 384, 0, 384, {}, {-1, 385}}};
  CHECK(sizeof(gmf::kKnobs) / sizeof(gmf::kKnobs[0]) == want.size());
  // what every knob reads from `t`, in the order of `want`
  auto snapshot = [&](const gmf::Tuning& t, std::vector<int>& out) {
    out.assign(want.size(), -12345);
    for (size_t i = 0; i < want.size(); ++i)
      if (!gmf::get_knob(t, want[i].name, &out[i])) return false;
    return true;
  };
  std::vector<int> defaults, now;
  g_where = "defaults";
  CHECK(snapshot(gmf::Tuning{}, defaults));
  for (size_t i = 0; i < want.size(); ++i) {
    const KnobWant& k = want[i];
    g_where = k.name;
    CHECK(defaults[i] == k.def);
    std::vector<int> accepted = k.only;
    for (int v = k.lo; v <= k.hi; ++v) accepted.push_back(v);
    CHECK(!accepted.empty());
    std::string why;
    for (int v : accepted) {
      gmf::Tuning t;
      CHECK(gmf::set_knob(t, k.name, v, &why) && why.empty());
      CHECK(snapshot(t, now));
      CHECK(now[i] == v);                                   // round trip, and no other knob moved
      now[i] = defaults[i];
      CHECK(now == defaults);
    }
    for (int v : k.refused) {
      gmf::Tuning t;
      why.clear();
      CHECK(!gmf::set_knob(t, k.name, v, &why));
      CHECK(why.find(k.name) != std::string::npos && why.find("unknown") == std::string::npos);
      CHECK(why.find(std::to_string(accepted.front())) != std::string::npos && why.find(std::to_string(accepted.back())) != std::string::npos);
      CHECK(snapshot(t, now) && now == defaults);           // refused: nothing changed
    }
  }
  g_where = "unknown knob";
  gmf::Tuning t;
  std::string why;
  int v = 77;
  CHECK(!gmf::set_knob(t, "no_such_knob", 1, &why) && why == "unknown knob no_such_knob");
  CHECK(!gmf::get_knob(t, "no_such_knob", &v) && v == 77);
  CHECK(!gmf::set_knob(t, "", 1, &why) && !gmf::get_knob(t, "kv_fol", &v) && !gmf::get_knob(t, "kv_fold ", &v));
  CHECK(snapshot(t, now) && now == defaults);
  return 0;
}

int main() {
  if (table()) return 1;
  if (knobs()) return 1;
  std::printf("encoder_plan_host: ok\n");
  return 0;
}
