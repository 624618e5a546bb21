// wpt_photon.cpp — host build of the PNEE octree (see wpt_photon.h).
#include "wpt_photon.h"

namespace wpt {

PhotonTree::PhotonTree(uint32_t num_lights) : num_lights_(num_lights) {
  nodes_.resize(1);
  nodes_[0].bins.assign(num_lights_, 1.0f);  // EmpiricalPDF::new (empirical_pdf.rs:22-28)
}

void PhotonTree::insert(uint32_t light, V3 loc, float intensity) {
  const float b[6] = {-kPhotonTreeSize, -kPhotonTreeSize, -kPhotonTreeSize,
                      kPhotonTreeSize,  kPhotonTreeSize,  kPhotonTreeSize};
  insert_at(0, b, PhotonRec{light, loc, intensity}, 0);
  inserted_++;
}

// Octree::insert (photon_tree.rs:171-206). `depth` only guards the split:
// more than 1024 photons at one point would make the reference recurse
// without end; here such a cell stops splitting below depth 120.
void PhotonTree::insert_at(uint32_t node, const float bounds[6], const PhotonRec& p, int depth) {
  nodes_[node].bins[p.light] += p.intensity;  // EmpiricalPDF::add
  if (nodes_[node].child != 0) {
    float cb[6];
    const uint32_t ci = octant(bounds, p.loc, cb);
    insert_at(nodes_[node].child + ci, cb, p, depth + 1);
    return;
  }
  nodes_[node].values.push_back(p);
  if (nodes_[node].values.size() > kMaxPhotonsInCell && depth < 120) {
    // split: a fresh internal node (bins = 1.0) over 8 empty leaves, then
    // every photon of the cell re-inserted in order
    std::vector<PhotonRec> vals;
    vals.swap(nodes_[node].values);
    const uint32_t first = (uint32_t)nodes_.size();
    nodes_.resize(nodes_.size() + 8);
    for (uint32_t c = 0; c < 8; c++) nodes_[first + c].bins.assign(num_lights_, 1.0f);
    nodes_[node].child = first;
    nodes_[node].bins.assign(num_lights_, 1.0f);
    for (const PhotonRec& v : vals) insert_at(node, bounds, v, depth);
  }
}

// EmpiricalPDF::recheck_cdf (empirical_pdf.rs:79-93), once per node.
void PhotonTree::freeze(std::vector<uint32_t>& child, std::vector<float>& cum) const {
  child.resize(nodes_.size());
  cum.assign(nodes_.size() * num_lights_, 0.0f);
  for (size_t i = 0; i < nodes_.size(); i++) {
    child[i] = nodes_[i].child;
    const std::vector<float>& b = nodes_[i].bins;
    float sum = 0.0f;
    for (float v : b) sum += v;
    float* c = cum.data() + i * num_lights_;
    if (num_lights_ == 0) continue;
    c[0] = 0.0f;
    for (uint32_t k = 1; k < num_lights_; k++) c[k] = c[k - 1] + b[k - 1] / sum;
  }
}

void oct_corner_table(const std::vector<uint32_t>& child, std::vector<uint32_t>& corners) {
  const size_t nn = child.size();
  corners.assign(64 * nn, 0u);
  auto walk = [&](uint32_t ix, uint32_t iy, uint32_t iz, int d) {
    uint32_t node = 0;
    for (int l = d - 1; l >= 0; l--) {
      const uint32_t c = child[node];
      if (c == 0u) break;
      node = c + (((ix >> l) & 1u) << 2) + (((iy >> l) & 1u) << 1) + ((iz >> l) & 1u);
    }
    return node;
  };
  struct Item {
    uint32_t node;
    int d;
    uint32_t kx, ky, kz;
  };
  std::vector<Item> todo{{0u, 0, 0u, 0u, 0u}};
  while (!todo.empty()) {
    const Item it = todo.back();
    todo.pop_back();
    const uint32_t c0 = child[it.node];
    if (c0 != 0u) {
      if (it.d < kOctLattice)
        for (uint32_t j = 0; j < 8; j++)
          todo.push_back({c0 + j, it.d + 1, 2 * it.kx + ((j >> 2) & 1u), 2 * it.ky + ((j >> 1) & 1u),
                          2 * it.kz + (j & 1u)});
      continue;
    }
    const int64_t last = ((int64_t)1 << it.d) - 1;
    auto adj = [&](uint32_t k, int off) {
      const int64_t a = (int64_t)k + off;
      return (uint32_t)(a < 0 ? 0 : (a > last ? last : a));
    };
    for (uint32_t oc = 0; oc < 8; oc++) {
      const uint32_t ax = adj(it.kx, (oc & 4u) ? 1 : -1), ay = adj(it.ky, (oc & 2u) ? 1 : -1),
                     az = adj(it.kz, (oc & 1u) ? 1 : -1);
      uint32_t* row = corners.data() + 64 * (size_t)it.node + 8 * oc;
      row[0] = it.node;
      for (uint32_t c = 1; c < 8; c++)
        row[c] = walk((c & 4u) ? ax : it.kx, (c & 2u) ? ay : it.ky, (c & 1u) ? az : it.kz, it.d);
    }
  }
}

}  // namespace wpt
