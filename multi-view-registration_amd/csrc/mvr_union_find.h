// csrc/mvr_union_find.h -- the lock-free union-find of the connected-component kernels (mvr_denoise.hip: PointCloud::denoise;
// mvr_cluster.hip: pcl::EuclideanClusterExtraction): parent[] over 32-bit node ids, every node its own parent at the start.
// The larger root is hooked under the smaller one with one atomicCAS, so the root a component ends with is its smallest
// node -- whatever the order of the unions and the shape of the launch.  Finds halve their path as they go: any ancestor is
// a valid parent, so the relaxed stores of concurrent finds never break a tree.  Not installed.
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace mvr {

__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x)
{
  for (;;) {
    const uint32_t p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED);
    if (p == x) return x;
    const uint32_t gp = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
    if (gp != p) __atomic_store_n(&parent[x], gp, __ATOMIC_RELAXED);       // path halving: any ancestor is a valid parent
    x = p;
  }
}

__device__ __forceinline__ void uf_unite(uint32_t *parent, uint32_t a, uint32_t b)
{
  for (;;) {
    a = uf_find(parent, a); b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    if (atomicCAS(&parent[a], a, b) == a) return;             // the larger root goes under the smaller one
  }
}

// One round of pointer jumping for node i: it adopts its grandparent.  All depths halve at once, with independent
// gathers instead of the dependent walk of a find -- the object is one giant component whose tree comes out of the
// union pass thousands of links deep, and 200k concurrent finds through it took 2.3 ms.
__device__ __forceinline__ void uf_jump(uint32_t *parent, size_t i)
{
  const uint32_t p = __atomic_load_n(&parent[i], __ATOMIC_RELAXED);
  const uint32_t gp = __atomic_load_n(&parent[p], __ATOMIC_RELAXED);
  if (gp != p) __atomic_store_n(&parent[i], gp, __ATOMIC_RELAXED);       // any ancestor is a valid parent
}

}  // namespace mvr
