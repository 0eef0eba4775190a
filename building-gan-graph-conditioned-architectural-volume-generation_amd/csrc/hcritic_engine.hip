// VoxelGNNDiscriminator.score_labels on the f16 kernels issued from C++:
// vg_hcritic_score (include/vgan.h).
//
// A restatement of vgan/half.py HalfCritic.score_labels(native=False): the
// eval forward of the critic (models.py:158-245 of the reference) over
// `copies` stacked candidate labellings.  Every launch is the library's own
// extern "C" entry point with the arguments the Python path passes, in its
// order, so the scores are bit-identical to it; the block-diagonal stacked
// CSR, which the Python path takes from vgan.ops.CSR.stacked, is built here
// by the kernel the generator sweep uses (hengine.h) -- integer offsets, the
// same values.  The GAT blocks make hgen_engine.hip's choices.
#include <stdint.h>

#include "../../include/vgan.h"
#include "common.h"
#include "hengine.h"

namespace {

bool gat_width(int c) {
  const int ld = r8(c);
  return c >= 1 && (ld == 8 || ld == 16 || ld == 32 || ld == 64 || ld == 128);
}

// vg_hcritic_decode's shapes: H -> H/2 -> H/4 -> H/8 -> 1
bool decode_fused(const vg_hcritic_model* md) {
  if (md->n_dec != 4) return false;
  const int H = md->dec[0].in;
  return (H == 16 || H == 32 || H == 64 || H == 128) && md->dec[0].out == H / 2 && md->dec[1].out == H / 4 &&
         md->dec[2].out == H / 8 && md->dec[3].out == 1;
}

// every argument any launch below depends on, before the first one.
// ptrs: the device pointers too (not for the arena query, which reads none)
int validate(const vg_hcritic_model* md, const vg_hcritic_batch* bt, bool ptrs) {
  const int nl = md->n_mlp, nb = md->n_blocks, nd = md->n_dec;
  if (bt->n <= 0 || bt->copies <= 0 || bt->num_edges <= 0 || bt->feat < 1 || nl < 1 || nb < 1 || nd < 1 ||
      nl > VG_HGEN_MAX_LAYERS || nb > VG_HGEN_MAX_BLOCKS || nd > VG_HGEN_MAX_LAYERS || md->classes < 1 ||
      md->classes > 32 || (long long)bt->copies * bt->n > (1LL << 30) ||
      (long long)bt->copies * bt->num_edges > (1LL << 30))
    return VG_EINVAL;
  const vg_hcritic_linear& L0 = md->mlp[0];
  // the embedding takes 256 columns, the f16 GEMMs around it 128
  if (L0.out < 1 || L0.out > 256 || L0.out > 128 || L0.in != bt->feat + md->classes) return VG_EINVAL;
  if (bt->ld_mvx % 8 || bt->ld_mvx < r8(bt->feat) || L0.ldw % 8 || L0.ldw < r8(bt->feat)) return VG_EINVAL;
  if (bt->copy_stride < bt->n) return VG_EINVAL;
  int w = L0.out;
  for (int j = 1; j < nl; ++j) {
    const vg_hcritic_linear& L = md->mlp[j];
    if (L.in != w || L.out < 1 || L.out > 128 || L.ldw % 8 || L.ldw < r8(L.in)) return VG_EINVAL;
    w = L.out;
  }
  for (int b = 0; b < nb; ++b) {
    const vg_hgen_block& B = md->block[b];
    if (B.in != w || !gat_width(B.out) || B.ldw % 8 || B.ldw < r8(B.in)) return VG_EINVAL;
    w = B.out;
  }
  const bool fused = decode_fused(md);
  for (int j = 0; j < nd; ++j) {
    const vg_hcritic_linear& L = md->dec[j];
    if (L.in != w || L.out < 1 || L.out > 128) return VG_EINVAL;
    if (!fused && (L.ldw % 8 || L.ldw < r8(L.in))) return VG_EINVAL;
    w = L.out;
  }
  if (w != 1) return VG_EINVAL;
  if (!ptrs) return 0;
  if (!bt->row_ptr || !bt->col || !bt->mvx || !bt->pred || (reinterpret_cast<uintptr_t>(bt->mvx) & 15))
    return VG_EINVAL;
  for (int j = 0; j < nl; ++j)
    if (!md->mlp[j].weight || (reinterpret_cast<uintptr_t>(md->mlp[j].weight) & 15)) return VG_EINVAL;
  if (!L0.weight_f32) return VG_EINVAL;
  for (int b = 0; b < nb; ++b) {
    const vg_hgen_block& B = md->block[b];
    if (!B.lin_weight || (reinterpret_cast<uintptr_t>(B.lin_weight) & 15) || !B.att_src || !B.att_dst || !B.bias ||
        !B.gn_weight || !B.gn_bias || !B.gn_mean_scale)
      return VG_EINVAL;
  }
  for (int j = 0; j < nd; ++j) {
    const vg_hcritic_linear& L = md->dec[j];
    if (fused ? !L.weight_f32 : (!L.weight || (reinterpret_cast<uintptr_t>(L.weight) & 15))) return VG_EINVAL;
  }
  return 0;
}

int run(Arena& ar, const vg_hcritic_model* md, const vg_hcritic_batch* bt, float* scores, double* score,
        int32_t* best, int8_t* labels, hipStream_t s) {
  if (const int rc = validate(md, bt, !ar.dry)) return rc;
  const int n = bt->n, kk = bt->copies, rows = kk * n;
  const int nl = md->n_mlp, nb = md->n_blocks, nd = md->n_dec;
  const vg_hcritic_linear& L0 = md->mlp[0];
  const int F = bt->feat, H = L0.out, ldb = r8(H);

  // the copy-invariant columns [matched | voxel.x] of the first Linear, bias
  // included, once on n rows; the label columns per candidate
  float* base = ar.take<float>((int64_t)n * ldb);
  VG_RUN(vg_hgemm(bt->mvx, bt->ld_mvx, L0.weight, L0.ldw, n, H, r8(F), L0.bias, 0, 0.f, base, ldb, 1, s));
  uint16_t* x0 = ar.take<uint16_t>((int64_t)rows * ldb);
  VG_RUN(vg_hcritic_embed_labels(base, ldb, L0.weight_f32, L0.in, F, md->classes, bt->pred, bt->copy_stride, kk, n, H,
                                 x0, ldb, s));
  const uint16_t* x = x0;
  int ldx = ldb;
  for (int j = 1; j < nl; ++j) {
    const vg_hcritic_linear& L = md->mlp[j];
    const int ldo = r8(L.out);
    uint16_t* out = ar.take<uint16_t>((int64_t)rows * ldo);
    VG_RUN(vg_hgemm(x, ldx, L.weight, L.ldw, rows, L.out, r8(L.in), L.bias, 1, 0.f, out, ldo, 0, s));
    x = out;
    ldx = ldo;
  }
  // GAT encoder over the stacked block-diagonal graph (one copy: the plain CSR)
  const int32_t* rp = bt->row_ptr;
  const int32_t* cl = bt->col;
  if (kk > 1) {
    int32_t* rps = ar.take<int32_t>((int64_t)rows + 1);
    int32_t* cls = ar.take<int32_t>((int64_t)kk * bt->num_edges);
    VG_RUN((k_hg_stack_csr<<<blocks_for((long long)rows + 1 + (long long)kk * bt->num_edges), 256, 0, s>>>(
                bt->row_ptr, bt->col, n, bt->num_edges, kk, rps, cls),
            launched()));
    rp = rps;
    cl = cls;
  }
  if (const int rc = run_gat_blocks(ar, s, md->block, nb, x, ldx, n, kk, rp, cl, nullptr, 0, &x, &ldx)) return rc;
  // decoder: one launch for the reference's halving widths, else per layer
  if (decode_fused(md)) {
    int32_t widths[5];
    const float* w[4];
    const float* bs[4];
    widths[0] = md->dec[0].in;
    for (int j = 0; j < 4; ++j) {
      widths[j + 1] = md->dec[j].out;
      w[j] = md->dec[j].weight_f32;
      bs[j] = md->dec[j].bias;
    }
    VG_RUN(vg_hcritic_decode(x, ldx, rows, widths, 4, w, bs, md->has_sigmoid, scores, s));
  } else {
    for (int j = 0; j < nd - 1; ++j) {
      const vg_hcritic_linear& L = md->dec[j];
      const int ldo = r8(L.out);
      uint16_t* out = ar.take<uint16_t>((int64_t)rows * ldo);
      VG_RUN(vg_hgemm(x, ldx, L.weight, L.ldw, rows, L.out, r8(L.in), L.bias, 1, 0.f, out, ldo, 0, s));
      x = out;
      ldx = ldo;
    }
    const vg_hcritic_linear& L = md->dec[nd - 1];
    VG_RUN(vg_hgemm(x, ldx, L.weight, L.ldw, rows, 1, r8(L.in), L.bias, 0, 0.f, scores, 1, 1, s));
    if (md->has_sigmoid) VG_RUN(vg_hcritic_sigmoid(scores, rows, s));
  }
  if (score)
    VG_RUN(vg_sweep_select_score(scores, n, bt->pred, bt->copy_stride, kk, bt->ptr, bt->num_graphs, n, score, best,
                                 labels, s));
  return 0;
}

}  // namespace

extern "C" int64_t vg_hcritic_arena_bytes(const vg_hcritic_model* model, const vg_hcritic_batch* batch) {
  if (!model || !batch) return VG_EINVAL;  // negative: an error, never a size
  Arena ar{true, nullptr};
  const int rc = run(ar, model, batch, nullptr, nullptr, nullptr, nullptr, nullptr);
  return rc ? (rc < 0 ? rc : -rc) : ar.off;
}

extern "C" int vg_hcritic_score(const vg_hcritic_model* model, const vg_hcritic_batch* batch, void* arena,
                                int64_t arena_bytes, float* scores, double* score, int32_t* best, int8_t* labels,
                                void* stream) {
  if (!model || !batch || !arena || !scores) return VG_EINVAL;
  const int given = (score != nullptr) + (best != nullptr) + (labels != nullptr);
  if (given != 0 && given != 3) return VG_EINVAL;
  if (given && (!batch->ptr || batch->num_graphs < 1)) return VG_EINVAL;
  const int64_t need = vg_hcritic_arena_bytes(model, batch);
  if (need < 0) return static_cast<int>(need);
  if (arena_bytes < need || (reinterpret_cast<uintptr_t>(arena) & 255)) return VG_EINVAL;
  Arena ar{false, static_cast<char*>(arena)};
  return run(ar, model, batch, scores, score, best, labels, static_cast<hipStream_t>(stream));
}
