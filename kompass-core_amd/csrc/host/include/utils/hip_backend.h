// RAII + exception bridge between the host C++ classes and the C ABI of
// libkompass_hip.so.  A failed call becomes the C++ exception type the
// reference would throw (std::invalid_argument / std::out_of_range /
// std::runtime_error); nothing here computes anything.
#pragma once

#include <memory>
#include <stdexcept>
#include <string>
#include <utility>

#include "kompass_hip.h"

namespace Kompass {
namespace hip {

inline void check(int rc) {
  if (rc == KC_OK) return;
  const std::string msg = kc_last_error();
  switch (rc) {
    case KC_ERR_INVALID: throw std::invalid_argument(msg);
    case KC_ERR_RANGE: throw std::out_of_range(msg);
    default: throw std::runtime_error(msg);
  }
}

// The one owner of a context of the library: a unique_ptr whose deleter is the context's destroy function.
template <class T, void (*Destroy)(T *)>
struct FnDeleter {
  void operator()(T *p) const { Destroy(p); }
};
template <class T, void (*Destroy)(T *)>
using Handle = std::unique_ptr<T, FnDeleter<T, Destroy>>;

using Dwa = Handle<kc_dwa, kc_dwa_destroy>;
using Comm = Handle<kc_comm, kc_comm_destroy>;
using MapperHandle = Handle<kc_mapper, kc_mapper_destroy>;
using CloudHandle = Handle<kc_cloud, kc_cloud_destroy>;
using ZoneHandle = Handle<kc_zone, kc_zone_destroy>;
using DepthHandle = Handle<kc_depth, kc_depth_destroy>;
using PlannerHandle = Handle<kc_planner, kc_planner_destroy>;
using WorldMapHandle = Handle<kc_worldmap, kc_worldmap_destroy>;
// The two shared contexts (sampler, evaluator and controller work on one kc_dwa): made from a Dwa / Comm, which
// keeps the context while the control block is allocated.
using DwaHandle = std::shared_ptr<kc_dwa>;
using CommHandle = std::shared_ptr<kc_comm>;

// create(args..., &raw), checked: the new context has its owner before anything can throw.
template <class H, class Create, class... Args>
H make(Create create, Args &&...args) {
  typename H::pointer raw = nullptr;
  const int rc = create(std::forward<Args>(args)..., &raw);
  H owner(raw);
  check(rc);
  return owner;
}

}  // namespace hip
}  // namespace Kompass
