// Python module `kompass_cpp` (pybind11; the reference uses nanobind, which is
// not installable offline -- SURVEY.md 8b).  Re-exposes the subset of the
// reference module that kompass_core.control.dwa / mapping.local_mapper and
// the named tests use, with the same submodule layout, class names, argument
// names and defaults (reference: src/kompass_cpp/bindings/*.cpp).
#include <cstring>
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "controllers/dwa.h"
#include "controllers/pure_pursuit.h"
#include "controllers/rgb_follower.h"
#include "controllers/rgbd_follower.h"
#include "controllers/mppi.h"
#include "controllers/stanley.h"
#include "mapping/local_mapper_gpu.h"
#include "mapping/mcl.h"
#include "mapping/mover_tracker.h"
#include "mapping/world_map.h"
#include "planning/grid_planner.h"
#include "utils/logger.h"
#include "utils/critical_zone_check.h"
#include "utils/pointcloud.h"
#include "vision/depth_detector.h"

namespace py = pybind11;
using namespace Kompass;

namespace {

using FArr = py::array_t<float, py::array::c_style | py::array::forcecast>;

Eigen::Vector3f vec3(const py::object &o) {
  auto a = py::cast<std::vector<float>>(o);
  if (a.size() != 3) throw std::invalid_argument("expected 3 values");
  return Eigen::Vector3f(a[0], a[1], a[2]);
}
Eigen::Vector4f vec4(const py::object &o) {
  auto a = py::cast<std::vector<float>>(o);
  if (a.size() != 4) throw std::invalid_argument("expected 4 values");
  return Eigen::Vector4f(a[0], a[1], a[2], a[3]);
}
std::vector<Path::Point> points(const py::object &o) {
  // list of 3-sequences or an (N,3) array
  FArr a = py::cast<FArr>(o);
  if (a.ndim() != 2 || a.shape(1) != 3) throw std::invalid_argument("expected an (N, 3) array of points");
  std::vector<Path::Point> out(static_cast<size_t>(a.shape(0)));
  auto r = a.unchecked<2>();
  for (py::ssize_t i = 0; i < a.shape(0); ++i) out[(size_t)i] = Path::Point(r(i, 0), r(i, 1), r(i, 2));
  return out;
}
using DArr = py::array_t<double, py::array::c_style | py::array::forcecast>;
// a 1-D float64 array as the std::vector<double> the reference signatures take: one memcpy (the element-wise
// sequence caster costs ~70 ns per beam)
std::vector<double> dvec(const DArr &a) {
  if (a.ndim() != 1) throw std::invalid_argument("expected a 1-D array");
  return std::vector<double>(a.data(), a.data() + a.size());
}
py::array_t<float> view1(const Eigen::VectorXf &v, py::handle owner) {
  return py::array_t<float>({(py::ssize_t)v.size()}, {(py::ssize_t)sizeof(float)}, v.data(), owner);
}
FArr copy1(const Eigen::VectorXf &v) {
  FArr a(v.size());
  std::memcpy(a.mutable_data(), v.data(), sizeof(float) * (size_t)v.size());
  return a;
}
Eigen::VectorXf toVec(const FArr &a) { return Eigen::VectorXf(a.data(), (Eigen::Index)a.size()); }

// vision types: fixed vectors as numpy arrays (int32 / float32), read and written whole
Eigen::Vector2i vec2i(const py::object &o) {
  auto a = py::cast<std::vector<int>>(o);
  if (a.size() != 2) throw std::invalid_argument("expected 2 values");
  return Eigen::Vector2i(a[0], a[1]);
}
Eigen::Vector2f vec2f(const py::object &o) {
  auto a = py::cast<std::vector<float>>(o);
  if (a.size() != 2) throw std::invalid_argument("expected 2 values");
  return Eigen::Vector2f(a[0], a[1]);
}
template <typename T, int N>
py::array_t<T> arr(const Eigen::FixedVec<T, N> &v) {
  py::array_t<T> a(N);
  std::memcpy(a.mutable_data(), v.data(), sizeof(T) * N);
  return a;
}
std::vector<Eigen::Vector2i> points2i(const py::object &o) {
  std::vector<Eigen::Vector2i> out;
  for (auto p : o) out.push_back(vec2i(py::reinterpret_borrow<py::object>(p)));
  return out;
}
std::vector<Eigen::Vector3f> points3f(const py::object &o) {
  std::vector<Eigen::Vector3f> out;
  for (auto p : o) out.push_back(vec3(py::reinterpret_borrow<py::object>(p)));
  return out;
}
template <typename T, int N>
py::list arrs(const std::vector<Eigen::FixedVec<T, N>> &v) {
  py::list l;
  for (const auto &x : v) l.append(arr(x));
  return l;
}
// a uint16 (H, W) numpy frame in any memory order, by pointer and strides (no copy)
DepthImageView depthView(const py::array &a) {
  if (!py::dtype::of<uint16_t>().is(a.dtype()) && a.dtype().num() != py::dtype::of<uint16_t>().num())
    throw py::type_error("depth_img must be a uint16 array, got " + py::str(a.dtype()).cast<std::string>());
  if (a.ndim() != 2) throw std::invalid_argument("depth_img must be 2-D (H, W)");
  DepthImageView v;
  v.data = static_cast<const uint16_t *>(a.data());
  v.rows = a.shape(0);
  v.cols = a.shape(1);
  v.row_stride = a.strides(0) / static_cast<py::ssize_t>(sizeof(uint16_t));
  v.col_stride = a.strides(1) / static_cast<py::ssize_t>(sizeof(uint16_t));
  if (a.strides(0) % 2 || a.strides(1) % 2) throw std::invalid_argument("depth_img strides must be whole elements");
  return v;
}

// A depth frame for the followers: a uint16 (H, W) numpy array (depthView), or an object that already lives on the
// device and exposes __cuda_array_interface__ (a torch ROCm tensor, ...), read in place.  `stream` is what the read
// must wait for: the interface's `stream` (1 = the legacy default stream, 2 = per-thread default, else a
// hipStream_t); an interface without the key (version 2, as torch writes it) means the legacy default stream; an
// explicit None means no wait.
// A host frame that is not an ndarray (an __array_interface__ object, an __array__ that copies) is converted, and
// the frame keeps that array alive for as long as the view is read.
struct DepthFrame {
  DepthImageView view;
  bool wait = false;
  void *stream = nullptr;
  py::array host;  // owner of view.data for a host frame
};
DepthFrame depthFrame(const py::object &o) {
  DepthFrame f;
  if (!py::hasattr(o, "__cuda_array_interface__")) {
    f.host = py::cast<py::array>(o);
    f.view = depthView(f.host);
    return f;
  }
  const py::dict d = o.attr("__cuda_array_interface__");
  const std::string ts = py::cast<std::string>(d["typestr"]);
  if (ts != "<u2" && ts != "|u2" && ts != "=u2")
    throw py::type_error("depth_img must be a uint16 array, got typestr " + ts);
  const auto shape = py::cast<std::vector<int64_t>>(d["shape"]);
  if (shape.size() != 2) throw std::invalid_argument("depth_img must be 2-D (H, W)");
  if (d.contains("mask") && !d["mask"].is_none()) throw std::invalid_argument("masked depth frames are not supported");
  f.view.rows = shape[0];
  f.view.cols = shape[1];
  f.view.row_stride = shape[1];
  f.view.col_stride = 1;
  if (d.contains("strides") && !d["strides"].is_none()) {
    const auto st = py::cast<std::vector<int64_t>>(d["strides"]);
    if (st.size() != 2 || st[0] % 2 || st[1] % 2) throw std::invalid_argument("depth_img strides must be whole elements");
    f.view.row_stride = st[0] / 2;
    f.view.col_stride = st[1] / 2;
  }
  const py::tuple data = d["data"];
  f.view.data = reinterpret_cast<const uint16_t *>(static_cast<uintptr_t>(py::cast<uint64_t>(data[0])));
  f.view.on_device = true;
  f.wait = true;
  if (d.contains("stream")) {
    const py::object s = d["stream"];
    if (s.is_none()) {
      f.wait = false;
    } else {
      const uint64_t h = py::cast<uint64_t>(s);
      if (h == 0) throw std::invalid_argument("__cuda_array_interface__ stream 0 is not allowed");
      f.stream = h == 1 ? nullptr : reinterpret_cast<void *>(static_cast<uintptr_t>(h));
    }
  }
  return f;
}
py::object trackedState(const std::optional<Eigen::MatrixXf> &s) {
  if (!s) return py::none();
  FArr a(s->rows());
  for (Eigen::Index i = 0; i < s->rows(); ++i) a.mutable_at(i) = (*s)(i, 0);
  return a;
}

// (grid, origin) of the occupancy-grid calls: the int8 matrix moves to the heap and the (cells_x, cells_y)
// column-major array views it (grid[i, j] is the cell (i, j)); no copy
py::tuple gridResult(std::pair<OccupancyGridI8, std::array<float, 3>> &&r) {
  auto *g = new OccupancyGridI8(std::move(r.first));
  py::capsule owner(g, [](void *p) { delete static_cast<OccupancyGridI8 *>(p); });
  py::array_t<int8_t> a({(py::ssize_t)g->rows(), (py::ssize_t)g->cols()},
                        {(py::ssize_t)1, (py::ssize_t)std::max<Eigen::Index>(g->rows(), 1)}, g->data(), owner);
  return py::make_tuple(a, py::make_tuple(r.second[0], r.second[1], r.second[2]));
}
void checkResolution(float grid_resolution) {
  if (!(grid_resolution > 0.0f) || !std::isfinite(grid_resolution))
    throw py::value_error("grid_resolution must be a positive finite float");
}
// points_to_occupancy_grid: an (N, 3) float32 cloud on the host (any array-like) or on the device (an object
// with __cuda_array_interface__, read in place after the work queued on its stream: cf. depthFrame)
py::tuple pointsToGrid(const py::object &o, float grid_resolution, float z_ground_limit, float robot_height) {
  checkResolution(grid_resolution);
  if (!py::hasattr(o, "__cuda_array_interface__")) {
    const FArr a = py::cast<FArr>(o);
    if (a.ndim() != 2 || a.shape(1) != 3) throw std::invalid_argument("expected an (N, 3) array of points");
    const size_t n = static_cast<size_t>(a.shape(0));
    const int8_t *data = reinterpret_cast<const int8_t *>(a.data());
    std::pair<OccupancyGridI8, std::array<float, 3>> r;
    {
      py::gil_scoped_release nogil;
      r = pointsToOccupancyGrid(data, n * 12, false, 12, n, 0, 4, 8, grid_resolution, z_ground_limit, robot_height);
    }
    return gridResult(std::move(r));
  }
  const py::dict d = o.attr("__cuda_array_interface__");
  const std::string ts = py::cast<std::string>(d["typestr"]);
  if (ts != "<f4" && ts != "=f4") throw py::type_error("points must be a float32 array, got typestr " + ts);
  const auto shape = py::cast<std::vector<int64_t>>(d["shape"]);
  if (shape.size() != 2 || shape[1] != 3) throw std::invalid_argument("expected an (N, 3) array of points");
  if (d.contains("mask") && !d["mask"].is_none()) throw std::invalid_argument("masked clouds are not supported");
  int64_t s0 = 12, s1 = 4;
  if (d.contains("strides") && !d["strides"].is_none()) {
    const auto st = py::cast<std::vector<int64_t>>(d["strides"]);
    if (st.size() != 2) throw std::invalid_argument("points strides must match the shape");
    s0 = st[0];
    s1 = st[1];
  }
  const size_t n = static_cast<size_t>(shape[0]);
  if (n == 0) s0 = 12, s1 = 4;  // nothing is read: whatever strides a producer reports for no rows
  if (s1 < 4 || s0 < 2 * s1 + 4 || s0 > 0x7FFFFFFF)
    throw std::invalid_argument("points must be records of x, y, z at increasing offsets (positive strides)");
  const py::tuple data = d["data"];
  const int8_t *ptr = reinterpret_cast<const int8_t *>(static_cast<uintptr_t>(py::cast<uint64_t>(data[0])));
  bool wait = true;
  void *stream = nullptr;
  if (d.contains("stream")) {
    const py::object s = d["stream"];
    if (s.is_none()) {
      wait = false;
    } else {
      const uint64_t h = py::cast<uint64_t>(s);
      if (h == 0) throw std::invalid_argument("__cuda_array_interface__ stream 0 is not allowed");
      stream = h == 1 ? nullptr : reinterpret_cast<void *>(static_cast<uintptr_t>(h));
    }
  }
  std::pair<OccupancyGridI8, std::array<float, 3>> r;
  {
    py::gil_scoped_release nogil;
    const size_t nbytes = n ? (n - 1) * static_cast<size_t>(s0) + static_cast<size_t>(2 * s1 + 4) : 0;
    r = pointsToOccupancyGrid(ptr, nbytes, true, static_cast<int>(s0), n, 0, static_cast<int>(s1),
                              static_cast<int>(2 * s1), grid_resolution, z_ground_limit, robot_height, wait, stream);
  }
  return gridResult(std::move(r));
}

// GridPlanner.set_grid: a (width, height) int32 or int8 grid, grid[i, j] the cell (i, j) -- a numpy array (any
// memory order; one copy when it is not column-major already), or an object that lives on the device and exposes
// __cuda_array_interface__ with that shape in column-major strides (the transpose of a C-contiguous (height,
// width) torch tensor), read in place
void plannerSetGrid(Planning::GridPlanner &p, const py::object &o) {
  if (!py::hasattr(o, "__cuda_array_interface__")) {
    const py::array a = py::cast<py::array>(o);
    if (a.ndim() != 2) throw std::invalid_argument("the grid must be 2-D (width, height)");
    if (a.dtype().num() == py::dtype::of<int8_t>().num()) {
      const auto g = py::array_t<int8_t, py::array::f_style>::ensure(a);
      p.setSpaceBoundsCheck(static_cast<int>(g.shape(0)), static_cast<int>(g.shape(1)));
      const void *d = g.data();
      py::gil_scoped_release nogil;
      p.setGrid(d, 1);
    } else if (a.dtype().num() == py::dtype::of<int32_t>().num()) {
      const auto g = py::array_t<int32_t, py::array::f_style>::ensure(a);
      p.setSpaceBoundsCheck(static_cast<int>(g.shape(0)), static_cast<int>(g.shape(1)));
      const void *d = g.data();
      py::gil_scoped_release nogil;
      p.setGrid(d, 4);
    } else {
      throw py::type_error("the grid must be int32 or int8, got " + py::str(a.dtype()).cast<std::string>());
    }
    return;
  }
  const py::dict d = o.attr("__cuda_array_interface__");
  const std::string ts = py::cast<std::string>(d["typestr"]);
  int elem = 0;
  if (ts == "<i4" || ts == "=i4") elem = 4;
  else if (ts == "|i1" || ts == "<i1" || ts == "=i1") elem = 1;
  else throw py::type_error("the grid must be int32 or int8, got typestr " + ts);
  const auto shape = py::cast<std::vector<int64_t>>(d["shape"]);
  if (shape.size() != 2) throw std::invalid_argument("the grid must be 2-D (width, height)");
  if (d.contains("mask") && !d["mask"].is_none()) throw std::invalid_argument("masked grids are not supported");
  if (!d.contains("strides") || d["strides"].is_none()) {
    if (shape[0] != 1 && shape[1] != 1) throw std::invalid_argument("a device grid must be column-major: grid[i, j] at i + j * width");
  } else {
    const auto st = py::cast<std::vector<int64_t>>(d["strides"]);
    if (st.size() != 2 || (shape[0] > 1 && st[0] != elem) || (shape[1] > 1 && st[1] != elem * shape[0]))
      throw std::invalid_argument("a device grid must be column-major: grid[i, j] at i + j * width");
  }
  if (shape[0] > 0x7FFFFFFF || shape[1] > 0x7FFFFFFF) throw std::out_of_range("the grid is too large");
  p.setSpaceBoundsCheck(static_cast<int>(shape[0]), static_cast<int>(shape[1]));
  const py::tuple data = d["data"];
  const void *ptr = reinterpret_cast<const void *>(static_cast<uintptr_t>(py::cast<uint64_t>(data[0])));
  // the producer's stream must have finished the grid: wait for it as the interface asks
  if (!d.contains("stream") || !d["stream"].is_none()) {
    void *stream = nullptr;
    if (d.contains("stream")) {
      const uint64_t h = py::cast<uint64_t>(d["stream"]);
      if (h == 0) throw std::invalid_argument("__cuda_array_interface__ stream 0 is not allowed");
      stream = h == 1 ? nullptr : reinterpret_cast<void *>(static_cast<uintptr_t>(h));
    }
    p.waitForStream(stream);
  }
  py::gil_scoped_release nogil;
  p.setGridOnDevice(ptr, elem);
}

// WorldMap.device_grid: the cls plane where it lies, as an object with __cuda_array_interface__ -- (width, height)
// int8 in column-major strides, the form GridPlanner.set_grid reads in place.  `stream` is None: the map is
// finished whenever no call on it is running.  Keeps the map alive.
struct WorldMapDeviceGrid {
  py::object map;
  uint64_t ptr;
  int width, height;
};
py::dict worldMapInterface(const WorldMapDeviceGrid &g) {
  py::dict d;
  d["shape"] = py::make_tuple(g.width, g.height);
  d["typestr"] = "|i1";
  d["data"] = py::make_tuple(g.ptr, false);
  d["strides"] = py::make_tuple(1, g.width);
  d["version"] = 3;
  d["stream"] = py::none();
  return d;
}

// WorldMap.match: the record of one match and, through the map it keeps alive, its score table
struct WorldMapMatch {
  Mapping::WorldMap::Match m;
  py::object map;
  uint64_t number;
};
py::array worldMapMatchScores(const WorldMapMatch &r) {
  const auto &m = r.map.cast<const Mapping::WorldMap &>();
  if (m.matchCount() != r.number) throw std::runtime_error("the map has made another match since: its table has replaced this one");
  const py::ssize_t nr = 2 * r.m.n_yaw + 1, side = 2 * r.m.reach + 1;
  std::vector<uint32_t> v;
  {
    py::gil_scoped_release nogil;
    v = m.matchScores();
  }
  py::array_t<uint32_t> a({nr, side, side});
  if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(uint32_t));
  return a;
}
kc_worldmap_pose worldMapPose(const py::tuple &t) {
  if (t.size() != 4) throw std::invalid_argument("a quantised pose is (cq, sq, tx, ty)");
  return kc_worldmap_pose{py::cast<int32_t>(t[0]), py::cast<int32_t>(t[1]), py::cast<int64_t>(t[2]), py::cast<int64_t>(t[3])};
}
const py::array_t<int32_t, py::array::f_style> worldMapLocalGrid(const py::array &grid) {
  if (grid.ndim() != 2 || grid.dtype().num() != py::dtype::of<int32_t>().num())
    throw std::invalid_argument("the local grid must be a 2-D int32 array (grid_height, grid_width)");
  return py::array_t<int32_t, py::array::f_style>::ensure(grid);
}

// WorldMap.set_prior: a (width, height) int32 or int8 grid, grid[I, J] the cell (I, J) -- a numpy array (any memory
// order), or a device array with __cuda_array_interface__ in column-major strides, read in place (cf. plannerSetGrid)
void worldMapSetPrior(Mapping::WorldMap &m, const py::object &o) {
  if (!py::hasattr(o, "__cuda_array_interface__")) {
    const py::array a = py::cast<py::array>(o);
    if (a.ndim() != 2) throw std::invalid_argument("the prior must be 2-D (width, height)");
    const int w = static_cast<int>(a.shape(0)), h = static_cast<int>(a.shape(1));
    if (a.dtype().num() == py::dtype::of<int8_t>().num()) {
      const auto g = py::array_t<int8_t, py::array::f_style>::ensure(a);
      const void *d = g.data();
      py::gil_scoped_release nogil;
      m.setPrior(d, 1, w, h);
    } else if (a.dtype().num() == py::dtype::of<int32_t>().num()) {
      const auto g = py::array_t<int32_t, py::array::f_style>::ensure(a);
      const void *d = g.data();
      py::gil_scoped_release nogil;
      m.setPrior(d, 4, w, h);
    } else {
      throw py::type_error("the prior must be int32 or int8, got " + py::str(a.dtype()).cast<std::string>());
    }
    return;
  }
  const py::dict d = o.attr("__cuda_array_interface__");
  const std::string ts = py::cast<std::string>(d["typestr"]);
  int elem = 0;
  if (ts == "<i4" || ts == "=i4") elem = 4;
  else if (ts == "|i1" || ts == "<i1" || ts == "=i1") elem = 1;
  else throw py::type_error("the prior must be int32 or int8, got typestr " + ts);
  const auto shape = py::cast<std::vector<int64_t>>(d["shape"]);
  if (shape.size() != 2) throw std::invalid_argument("the prior must be 2-D (width, height)");
  if (d.contains("mask") && !d["mask"].is_none()) throw std::invalid_argument("masked grids are not supported");
  if (!d.contains("strides") || d["strides"].is_none()) {
    if (shape[0] != 1 && shape[1] != 1) throw std::invalid_argument("a device prior must be column-major: grid[I, J] at I + J * width");
  } else {
    const auto st = py::cast<std::vector<int64_t>>(d["strides"]);
    if (st.size() != 2 || (shape[0] > 1 && st[0] != elem) || (shape[1] > 1 && st[1] != elem * shape[0]))
      throw std::invalid_argument("a device prior must be column-major: grid[I, J] at I + J * width");
  }
  if (shape[0] > 0x7FFFFFFF || shape[1] > 0x7FFFFFFF) throw std::out_of_range("the prior is too large");
  const py::tuple data = d["data"];
  const void *ptr = reinterpret_cast<const void *>(static_cast<uintptr_t>(py::cast<uint64_t>(data[0])));
  if (!d.contains("stream") || !d["stream"].is_none()) {
    void *stream = nullptr;
    if (d.contains("stream")) {
      const uint64_t h = py::cast<uint64_t>(d["stream"]);
      if (h == 0) throw std::invalid_argument("__cuda_array_interface__ stream 0 is not allowed");
      stream = h == 1 ? nullptr : reinterpret_cast<void *>(static_cast<uintptr_t>(h));
    }
    m.waitForStream(stream);
  }
  py::gil_scoped_release nogil;
  m.setPriorOnDevice(ptr, elem, static_cast<int>(shape[0]), static_cast<int>(shape[1]));
}

void fromDict(Parameters &p, const py::dict &d) {
  for (auto item : d) {
    const std::string name = py::cast<std::string>(item.first);
    auto it = p.parameters.find(name);
    if (it == p.parameters.end()) continue;
    try {
      py::handle v = item.second;
      if (py::isinstance<py::bool_>(v)) it->second.setValue(py::cast<bool>(v));
      else if (py::isinstance<py::float_>(v)) it->second.setValue(py::cast<double>(v));
      else if (py::isinstance<py::str>(v)) it->second.setValue(py::cast<std::string>(v));
      else if (py::isinstance<py::int_>(v)) it->second.setValue(py::cast<int>(v));
    } catch (const std::exception &e) {
      throw std::runtime_error(e.what());
    }
  }
}

}  // namespace

PYBIND11_MODULE(kompass_cpp, m) {
  m.doc() = "Algorithms for robot path tracking and control (MI355X / HIP build of the hot path)";

  // ---------------------------------------------------------------- types
  auto t = m.def_submodule("types", "KOMPASS CPP data types module");
  py::enum_<Path::InterpolationType>(t, "PathInterpolationType")
      .value("LINEAR", Path::InterpolationType::LINEAR)
      .value("CUBIC_SPLINE", Path::InterpolationType::CUBIC_SPLINE)
      .value("HERMITE_SPLINE", Path::InterpolationType::HERMITE_SPLINE)
      .export_values();

  py::class_<Path::State>(t, "State")
      .def(py::init<double, double, double, double>(), py::arg("x") = 0.0, py::arg("y") = 0.0,
           py::arg("yaw") = 0.0, py::arg("speed") = 0.0)
      .def_readwrite("x", &Path::State::x)
      .def_readwrite("y", &Path::State::y)
      .def_readwrite("yaw", &Path::State::yaw)
      .def_readwrite("speed", &Path::State::speed);

  py::class_<Path::PathPosition>(t, "PathPosition")
      .def(py::init<>())
      .def_readwrite("segment_index", &Path::PathPosition::segment_index)
      .def_readwrite("segment_length", &Path::PathPosition::segment_length)
      .def_readwrite("parallel_distance", &Path::PathPosition::parallel_distance)
      .def_readwrite("normal_distance", &Path::PathPosition::normal_distance);

  py::class_<Path::Path>(t, "Path")
      .def(py::init([](const py::object &pts) { return Path::Path(points(pts)); }), py::arg("points"))
      .def("reached_end", &Path::Path::endReached)
      .def("get_total_length", &Path::Path::totalPathLength)
      .def("size", &Path::Path::getSize)
      .def("getIndex", [](const Path::Path &p, size_t i) {
             const Path::Point q = p.getIndex(i);
             FArr a(3);
             a.mutable_at(0) = q.x(); a.mutable_at(1) = q.y(); a.mutable_at(2) = q.z();
             return a;
           }, py::arg("index"))
      .def("x", [](const Path::Path &p) { return copy1(p.getX()); })
      .def("y", [](const Path::Path &p) { return copy1(p.getY()); });

  py::class_<Control::Velocity2D>(t, "Velocity2D")
      .def(py::init([](float vx, float vy, float omega, float steer) {
             return Control::Velocity2D(vx, vy, omega, steer);
           }), py::arg("vx") = 0.0, py::arg("vy") = 0.0, py::arg("omega") = 0.0, py::arg("steer_ang") = 0.0)
      .def_property("vx", &Control::Velocity2D::vx, &Control::Velocity2D::setVx)
      .def_property("vy", &Control::Velocity2D::vy, &Control::Velocity2D::setVy)
      .def_property("omega", &Control::Velocity2D::omega, &Control::Velocity2D::setOmega)
      .def_property("steer_ang", &Control::Velocity2D::steer_ang, &Control::Velocity2D::setSteerAng)
      .def("__str__", [](const Control::Velocity2D &v) {
        return "{" + std::to_string(v.vx()) + ", " + std::to_string(v.vy()) + ", " + std::to_string(v.omega()) + "})";
      });

  py::class_<Control::TrajectoryVelocities2D>(t, "TrajectoryVelocities2D")
      .def(py::init<>())
      .def(py::init([](size_t length) { return Control::TrajectoryVelocities2D(length + 1); }), py::arg("length"))
      .def(py::init<const std::vector<Control::Velocity2D> &>(), py::arg("velocities"))
      .def(py::init([](const FArr &vx, const FArr &vy, const FArr &om) {
             return Control::TrajectoryVelocities2D(toVec(vx), toVec(vy), toVec(om));
           }), py::arg("vx"), py::arg("vy"), py::arg("omega"))
      .def_property_readonly("vx", [](py::object self) {
             return view1(self.cast<const Control::TrajectoryVelocities2D &>().vx, self); })
      .def_property_readonly("vy", [](py::object self) {
             return view1(self.cast<const Control::TrajectoryVelocities2D &>().vy, self); })
      .def_property_readonly("omega", [](py::object self) {
             return view1(self.cast<const Control::TrajectoryVelocities2D &>().omega, self); })
      .def_property("length",
           [](const Control::TrajectoryVelocities2D &v) {
             return v.numPointsPerTrajectory_ > 0 ? v.numPointsPerTrajectory_ - 1 : 0; },
           [](Control::TrajectoryVelocities2D &v, size_t length) { v.numPointsPerTrajectory_ = length + 1; });

  py::class_<Control::TrajectoryPath>(t, "TrajectoryPath")
      .def(py::init<>())
      .def_property_readonly("x", [](py::object self) { return view1(self.cast<const Control::TrajectoryPath &>().x, self); })
      .def_property_readonly("y", [](py::object self) { return view1(self.cast<const Control::TrajectoryPath &>().y, self); })
      .def_property_readonly("z", [](py::object self) { return view1(self.cast<const Control::TrajectoryPath &>().z, self); });

  py::class_<Control::Trajectory2D>(t, "Trajectory")
      .def(py::init<>())
      .def_readonly("velocities", &Control::Trajectory2D::velocities)
      .def_readonly("path", &Control::Trajectory2D::path);

  py::class_<Control::LaserScan>(t, "LaserScan")
      // numpy arrays first (one memcpy each); lists and other sequences fall through to the element-wise form
      .def(py::init([](const py::array_t<double, py::array::c_style | py::array::forcecast> &ranges,
                       const py::array_t<double, py::array::c_style | py::array::forcecast> &angles) {
             if (ranges.ndim() != 1 || angles.ndim() != 1) throw std::invalid_argument("ranges and angles must be 1-D");
             return Control::LaserScan(std::vector<double>(ranges.data(), ranges.data() + ranges.size()),
                                       std::vector<double>(angles.data(), angles.data() + angles.size()));
           }), py::arg("ranges").noconvert(), py::arg("angles").noconvert())
      .def(py::init<std::vector<double>, std::vector<double>>(), py::arg("ranges"), py::arg("angles"))
      .def_readonly("ranges", &Control::LaserScan::ranges)
      .def_readonly("angles", &Control::LaserScan::angles);

  py::enum_<CollisionChecker::ShapeType>(t, "RobotGeometry")
      .value("CYLINDER", CollisionChecker::ShapeType::CYLINDER)
      .value("BOX", CollisionChecker::ShapeType::BOX)
      .value("SPHERE", CollisionChecker::ShapeType::SPHERE)
      .def_static("get", [](const std::string &key) {
        if (key == "CYLINDER") return CollisionChecker::ShapeType::CYLINDER;
        if (key == "BOX") return CollisionChecker::ShapeType::BOX;
        if (key == "SPHERE") return CollisionChecker::ShapeType::SPHERE;
        throw std::runtime_error("Invalid key");
      });


  // vision types (bindings_types.cpp:188-235)
  py::class_<PointsOfInterest>(t, "PointsOfInterest")
      .def(py::init<>())
      .def(py::init<const PointsOfInterest &>())
      .def(py::init([](const py::object &points, const py::object &img_size, float timestamp, const std::string &label) {
             return PointsOfInterest(points2i(points), vec2i(img_size), timestamp, label);
           }), py::arg("points"), py::arg("img_size") = std::vector<int>{640, 480}, py::arg("timestamp") = 0.0,
           py::arg("label") = "")
      .def_property("points_2d", [](const PointsOfInterest &p) { return arrs(p.Points2D); },
                    [](PointsOfInterest &p, const py::object &o) { p.Points2D = points2i(o); })
      .def_readwrite("timestamp", &PointsOfInterest::timestamp)
      .def_readwrite("label", &PointsOfInterest::label)
      .def_property("img_size", [](const PointsOfInterest &p) { return arr(p.img_size); },
                    [](PointsOfInterest &p, const py::object &o) { p.img_size = vec2i(o); })
      .def_property("vel", [](const PointsOfInterest &p) { return arr(p.vel); },
                    [](PointsOfInterest &p, const py::object &o) { p.vel = vec2i(o); })
      .def("set_vel", [](PointsOfInterest &p, const py::object &o) { p.setVel(vec2i(o)); })
      .def("set_img_size", [](PointsOfInterest &p, const py::object &o) { p.setImgSize(vec2i(o)); });

  py::class_<Bbox2D>(t, "Bbox2D")
      .def(py::init<>())
      .def(py::init<const Bbox2D &>())
      .def(py::init([](const py::object &top, const py::object &size, float timestamp, const std::string &label) {
             return Bbox2D(vec2i(top), vec2i(size), timestamp, label);
           }), py::arg("top_left_corner"), py::arg("size"), py::arg("timestamp") = 0.0, py::arg("label") = "")
      .def_property("top_left_corner", [](const Bbox2D &b) { return arr(b.top_corner); },
                    [](Bbox2D &b, const py::object &o) { b.top_corner = vec2i(o); })
      .def_property("size", [](const Bbox2D &b) { return arr(b.size); },
                    [](Bbox2D &b, const py::object &o) { b.size = vec2i(o); })
      .def_readwrite("timestamp", &Bbox2D::timestamp)
      .def_readwrite("label", &Bbox2D::label)
      .def_property("img_size", [](const Bbox2D &b) { return arr(b.img_size); },
                    [](Bbox2D &b, const py::object &o) { b.img_size = vec2i(o); })
      .def("set_vel", [](Bbox2D &b, const py::object &o) { b.setVel(vec3(o)); })
      .def("set_img_size", [](Bbox2D &b, const py::object &o) { b.setImgSize(vec2i(o)); });

  py::class_<Bbox3D>(t, "Bbox3D")
      .def(py::init<>())
      .def(py::init<const Bbox3D &>())
      .def(py::init([](const py::object &center, const py::object &size, const py::object &cimg,
                       const py::object &simg, float timestamp, const std::string &label, const py::object &pc) {
             return Bbox3D(vec3(center), vec3(size), vec2i(cimg), vec2i(simg), timestamp, label, points3f(pc));
           }), py::arg("center"), py::arg("size"), py::arg("center_img_frame"), py::arg("size_img_frame"),
           py::arg("timestamp") = 0.0, py::arg("label") = "", py::arg("pc_points") = py::list())
      .def_property("center", [](const Bbox3D &b) { return arr(b.center); },
                    [](Bbox3D &b, const py::object &o) { b.center = vec3(o); })
      .def_property("size", [](const Bbox3D &b) { return arr(b.size); },
                    [](Bbox3D &b, const py::object &o) { b.size = vec3(o); })
      .def_property("center_img_frame", [](const Bbox3D &b) { return arr(b.center_img_frame); },
                    [](Bbox3D &b, const py::object &o) { b.center_img_frame = vec2i(o); })
      .def_property("size_img_frame", [](const Bbox3D &b) { return arr(b.size_img_frame); },
                    [](Bbox3D &b, const py::object &o) { b.size_img_frame = vec2i(o); })
      .def_property("pc_points", [](const Bbox3D &b) { return arrs(b.pc_points); },
                    [](Bbox3D &b, const py::object &o) { b.pc_points = points3f(o); })
      .def_readwrite("timestamp", &Bbox3D::timestamp)
      .def_readwrite("label", &Bbox3D::label);

  // ------------------------------------------------------------ configure
  auto cfg = m.def_submodule("configure", "Configuration classes");
  py::class_<Parameters>(cfg, "ConfigParameters").def(py::init<>()).def("from_dict", &fromDict);

  // -------------------------------------------------------------- control
  auto c = m.def_submodule("control", "Control module");
  py::enum_<Control::ControlType>(c, "ControlType")
      .value("ACKERMANN", Control::ControlType::ACKERMANN)
      .value("DIFFERENTIAL_DRIVE", Control::ControlType::DIFFERENTIAL_DRIVE)
      .value("OMNI", Control::ControlType::OMNI);

  py::class_<Control::LinearVelocityControlParams>(c, "LinearVelocityControlParams")
      .def(py::init<double, double, double>(), py::arg("max_vel") = 0.0, py::arg("max_acc") = 0.0,
           py::arg("max_decel") = 0.0)
      .def_readwrite("max_vel", &Control::LinearVelocityControlParams::maxVel)
      .def_readwrite("max_acc", &Control::LinearVelocityControlParams::maxAcceleration)
      .def_readwrite("max_decel", &Control::LinearVelocityControlParams::maxDeceleration);

  py::class_<Control::AngularVelocityControlParams>(c, "AngularVelocityControlParams")
      .def(py::init<double, double, double, double>(), py::arg("max_ang") = M_PI, py::arg("max_omega") = 0.0,
           py::arg("max_acc") = 0.0, py::arg("max_decel") = 0.0)
      .def_readwrite("max_steer_ang", &Control::AngularVelocityControlParams::maxAngle)
      .def_readwrite("max_omega", &Control::AngularVelocityControlParams::maxOmega)
      .def_readwrite("max_acc", &Control::AngularVelocityControlParams::maxAcceleration)
      .def_readwrite("max_decel", &Control::AngularVelocityControlParams::maxDeceleration);

  py::class_<Control::ControlLimitsParams>(c, "ControlLimitsParams")
      .def(py::init<>())
      .def(py::init([](const Control::LinearVelocityControlParams &x, const Control::LinearVelocityControlParams &y,
                       const Control::AngularVelocityControlParams &w) {
             return Control::ControlLimitsParams(x, y, w);
           }), py::arg("vel_x_ctr_params") = Control::LinearVelocityControlParams(),
           py::arg("vel_y_ctr_params") = Control::LinearVelocityControlParams(),
           py::arg("omega_ctr_params") = Control::AngularVelocityControlParams())
      .def_readwrite("linear_x_limits", &Control::ControlLimitsParams::velXParams)
      .def_readwrite("linear_y_limits", &Control::ControlLimitsParams::velYParams)
      .def_readwrite("angular_limits", &Control::ControlLimitsParams::omegaParams);

  py::class_<Control::Controller>(c, "Controller")
      .def(py::init<>())
      .def("set_linear_ctr_limits", &Control::Controller::setLinearControlLimits)
      .def("set_angular_ctr_limits", &Control::Controller::setAngularControlLimits)
      .def("set_ctr_type", &Control::Controller::setControlType)
      .def("set_current_velocity", &Control::Controller::setCurrentVelocity)
      .def("set_current_state", py::overload_cast<const Path::State &>(&Control::Controller::setCurrentState))
      .def("set_current_state", py::overload_cast<double, double, double, double>(&Control::Controller::setCurrentState))
      .def("get_ctr_type", &Control::Controller::getControlType)
      .def("get_control", &Control::Controller::getControl);

  py::class_<Control::Controller::ControllerParameters, Parameters>(c, "ControllerParameters").def(py::init<>());
  py::class_<Control::Follower::FollowerParameters, Control::Controller::ControllerParameters>(c, "FollowerParameters")
      .def(py::init<>());

  py::class_<Control::Follower::Target>(c, "FollowingTarget")
      .def(py::init<>())
      .def_readwrite("segment_index", &Control::Follower::Target::segment_index)
      .def_readwrite("position_in_segment", &Control::Follower::Target::position_in_segment)
      .def_readwrite("movement", &Control::Follower::Target::movement)
      .def_readwrite("reverse", &Control::Follower::Target::reverse)
      .def_readwrite("lookahead", &Control::Follower::Target::lookahead)
      .def_readwrite("crosstrack_error", &Control::Follower::Target::crosstrack_error)
      .def_readwrite("heading_error", &Control::Follower::Target::heading_error);

  py::class_<Control::Follower, Control::Controller>(c, "Follower")
      .def(py::init<>())
      .def(py::init<Control::Follower::FollowerParameters>())
      .def("set_interpolation_type", &Control::Follower::setInterpolationType)
      .def("set_current_path", &Control::Follower::setCurrentPath, py::arg("path"), py::arg("interpolate") = true)
      .def("clear_current_path", &Control::Follower::clearCurrentPath)
      .def("is_goal_reached", &Control::Follower::isGoalReached)
      .def("get_vx_cmd", &Control::Follower::getLinearVelocityCmdX)
      .def("get_vy_cmd", &Control::Follower::getLinearVelocityCmdY)
      .def("get_omega_cmd", &Control::Follower::getAngularVelocityCmd)
      .def("get_steer_cmd", &Control::Follower::getSteeringAngleCmd)
      .def("get_tracked_target", &Control::Follower::getTrackedTarget)
      .def("get_current_path", &Control::Follower::getCurrentPath)
      .def("get_path_length", &Control::Follower::getPathLength)
      .def("has_path", &Control::Follower::hasPath);

  py::enum_<Control::Controller::Result::Status>(c, "FollowingStatus")
      .value("GOAL_REACHED", Control::Controller::Result::Status::GOAL_REACHED)
      .value("LOOSING_GOAL", Control::Controller::Result::Status::LOOSING_GOAL)
      .value("COMMAND_FOUND", Control::Controller::Result::Status::COMMAND_FOUND)
      .value("NO_COMMAND_POSSIBLE", Control::Controller::Result::Status::NO_COMMAND_POSSIBLE);
  py::class_<Control::Controller::Result>(c, "FollowingResult")
      .def(py::init<>())
      .def_readwrite("status", &Control::Controller::Result::status)
      .def_readwrite("velocity_command", &Control::Controller::Result::velocity_command);

  py::class_<Control::TrajSearchResult>(c, "SamplingControlResult")
      .def(py::init<>())
      .def_readwrite("is_found", &Control::TrajSearchResult::isTrajFound)
      .def_readwrite("cost", &Control::TrajSearchResult::trajCost)
      .def_readwrite("trajectory", &Control::TrajSearchResult::trajectory);

  py::class_<Control::CostEvaluator::TrajectoryCostsWeights, Parameters>(c, "TrajectoryCostWeights").def(py::init<>());
  py::class_<Control::TrajectorySampler::TrajectorySamplerParameters, Parameters>(c, "TrajectorySamplerParameters")
      .def(py::init<>());

  using DWA = Control::DWA;
  py::class_<DWA, Control::Follower>(c, "DWA")
      .def(py::init([](Control::ControlLimitsParams lim, Control::ControlType type, double dt, double ph, double ch,
                       int ml, int ma, CollisionChecker::ShapeType shape, std::vector<float> dims,
                       const py::object &spos, const py::object &srot, double res,
                       Control::CostEvaluator::TrajectoryCostsWeights w, int threads) {
             return std::make_unique<DWA>(lim, type, dt, ph, ch, ml, ma, shape, dims, vec3(spos), vec4(srot), res, w, threads);
           }), py::arg("control_limits"), py::arg("control_type"), py::arg("time_step"),
           py::arg("prediction_horizon"), py::arg("control_horizon"), py::arg("max_linear_samples"),
           py::arg("max_angular_samples"), py::arg("robot_shape_type"), py::arg("robot_dimensions"),
           py::arg("sensor_position_robot"), py::arg("sensor_rotation_robot"), py::arg("octree_resolution"),
           py::arg("cost_weights"), py::arg("max_num_threads") = 1)
      .def(py::init([](Control::TrajectorySampler::TrajectorySamplerParameters cfg, Control::ControlLimitsParams lim,
                       Control::ControlType type, CollisionChecker::ShapeType shape, std::vector<float> dims,
                       const py::object &spos, const py::object &srot,
                       Control::CostEvaluator::TrajectoryCostsWeights w, int threads) {
             return std::make_unique<DWA>(cfg, lim, type, shape, dims, vec3(spos), vec4(srot), w, threads);
           }), py::arg("config"), py::arg("control_limits"), py::arg("control_type"), py::arg("robot_shape_type"),
           py::arg("robot_dimensions"), py::arg("sensor_position_robot"), py::arg("sensor_rotation_robot"),
           py::arg("cost_weights"), py::arg("max_num_threads") = 1)
      .def("compute_velocity_commands", [](DWA &d, const Control::Velocity2D &v, const Control::LaserScan &s) {
             return d.computeVelocityCommandsSet<Control::LaserScan>(v, s); })
      // sensor data = the last grid of a LocalMapper, consumed where it lies on
      // the device (not in the reference: SURVEY 8f rank 4)
      .def("compute_velocity_commands", [](DWA &d, const Control::Velocity2D &v, const Mapping::LocalMapper &m) {
             return d.computeVelocityCommandsSet<Mapping::LocalMapper>(v, m); })
      // sensor data = the occupied cells of a WorldMap within sensor range of the robot, extracted on the
      // device (not in the reference: DESIGN.md 4.11 rules 16 to 19)
      .def("compute_velocity_commands", [](DWA &d, const Control::Velocity2D &v, const Mapping::WorldMap &m) {
             return d.computeVelocityCommandsSet<Mapping::WorldMap>(v, m); })
      .def("compute_velocity_commands", [](DWA &d, const Control::Velocity2D &v, const py::object &cloud) {
             // an (N, 3) float32 C-contiguous array is consumed where it lies; anything else (lists of
             // tuples, other dtypes) is converted first
             const FArr a = py::cast<FArr>(cloud);
             if (a.ndim() != 2 || a.shape(1) != 3) throw std::invalid_argument("expected an (N, 3) array of points");
             return d.computeVelocityCommandsSet<Control::PointCloudView>(
                 v, Control::PointCloudView{a.data(), static_cast<size_t>(a.shape(0))}); })
      .def("add_custom_cost", &DWA::addCustomCost)
      .def("get_debugging_samples", [](const DWA &d) {
             auto [x, y] = d.getDebuggingSamples();
             FArr ax({(py::ssize_t)x.rows(), (py::ssize_t)x.cols()}), ay({(py::ssize_t)y.rows(), (py::ssize_t)y.cols()});
             std::memcpy(ax.mutable_data(), x.data(), sizeof(float) * (size_t)x.size());
             std::memcpy(ay.mutable_data(), y.data(), sizeof(float) * (size_t)y.size());
             return py::make_tuple(ax, ay);
           })
      .def("debug_velocity_search", [](DWA &d, const Control::Velocity2D &v, const Control::LaserScan &s, bool drop) {
             d.debugVelocitySearch<Control::LaserScan>(v, s, drop); }, py::call_guard<py::gil_scoped_release>())
      .def("debug_velocity_search", [](DWA &d, const Control::Velocity2D &v, const py::object &cloud, bool drop) {
             auto pts = points(cloud);
             py::gil_scoped_release rel;
             d.debugVelocitySearch<std::vector<Path::Point>>(v, pts, drop); })
      .def("set_resolution", &DWA::resetOctreeResolution)
      .def("set_sensor_max_range", &DWA::setSensorMaxRange)
      // additions of this build (no counterpart in the reference: its DWA is one device)
      .def("enable_sharding", [](DWA &d, int rank, int world, const py::bytes &unique_id, int device, bool by_rows) {
             const std::string id = unique_id;
             if (id.size() != KC_COMM_ID_BYTES) throw std::invalid_argument("unique_id must be 128 bytes (comm_unique_id())");
             d.enableSharding(rank, world, reinterpret_cast<const uint8_t *>(id.data()), device,
                              by_rows ? KC_SHARD_ROWS : KC_SHARD_BLOCKS);
           }, py::arg("rank"), py::arg("world"), py::arg("unique_id"), py::arg("device") = 0, py::arg("by_rows") = true,
           "One DWA per process / GPU: shares of the sample lattice (dealt by trig row, or contiguous blocks) + ONE "
           "RCCL all-reduce(min) of the exchange record per cycle")
      .def("enable_sharding_shm", [](DWA &d, int rank, int world, const std::string &name, int device, bool by_rows) {
             d.enableShardingShm(rank, world, name, device, by_rows ? KC_SHARD_ROWS : KC_SHARD_BLOCKS);
           }, py::arg("rank"), py::arg("world"), py::arg("name"), py::arg("device") = 0, py::arg("by_rows") = true,
           "The same over the shared-memory rehearsal transport (ranks that share a GPU)")
      .def("disable_sharding", &DWA::disableSharding)
      .def("use_resident_path", &DWA::useResidentPath, py::arg("on"),
           "Tracked-segment tables from a device-resident copy of the path (saves host time, adds a kernel)");

  // Stanley (bindings_control.cpp:135-150)
  py::class_<Control::Stanley::StanleyParameters, Control::Follower::FollowerParameters>(c, "StanleyParameters")
      .def(py::init<>());
  py::class_<Control::Stanley, Control::Follower>(c, "Stanley")
      .def(py::init<>(), "Init Stanley follower with default parameters")
      .def(py::init<Control::Stanley::StanleyParameters>(), "Init Stanley follower with custom config")
      .def("compute_velocity_commands", &Control::Stanley::computeVelocityCommand)
      .def("execute", &Control::Stanley::execute)
      .def("set_robot_wheelbase", &Control::Stanley::setWheelBase);

  // MPPI over a WorldMap's distance plane (not in the reference)
  {
    using MPPI = Control::MPPI;
    py::class_<MPPI::Config>(c, "MPPIConfig")
        .def(py::init<>())
        .def_readwrite("samples", &MPPI::Config::samples)
        .def_readwrite("horizon", &MPPI::Config::horizon)
        .def_readwrite("window", &MPPI::Config::window)
        .def_readwrite("sigma_forward", &MPPI::Config::sigma_forward)
        .def_readwrite("sigma_lateral", &MPPI::Config::sigma_lateral)
        .def_readwrite("sigma_turn", &MPPI::Config::sigma_turn)
        .def_readwrite("lambda_", &MPPI::Config::lambda)
        .def_readwrite("w_shift", &MPPI::Config::w_shift)
        .def_readwrite("n_w", &MPPI::Config::n_w)
        .def_readwrite("hit_radius", &MPPI::Config::hit_radius)
        .def_readwrite("clearance", &MPPI::Config::clearance)
        .def_readwrite("clearance_weight", &MPPI::Config::clearance_weight)
        .def_readwrite("pen_far", &MPPI::Config::pen_far)
        .def_readwrite("pen_hit", &MPPI::Config::pen_hit)
        .def_readwrite("w_path", &MPPI::Config::w_path)
        .def_readwrite("w_goal", &MPPI::Config::w_goal)
        .def_readwrite("path_cap", &MPPI::Config::path_cap)
        .def_readwrite("reach", &MPPI::Config::reach)
        .def_readwrite("allow_reverse", &MPPI::Config::allow_reverse)
        .def_readwrite("min_turning_radius", &MPPI::Config::min_turning_radius)
        .def_readwrite("seed", &MPPI::Config::seed)
        .def_readwrite("mover_margin", &MPPI::Config::mover_margin)
        .def_readwrite("mover_weight", &MPPI::Config::mover_weight)
        .def_readwrite("mover_hit_penalty", &MPPI::Config::mover_hit_penalty)
        .def_readwrite("field_run_weight", &MPPI::Config::field_run_weight)
        .def_readwrite("field_goal_weight", &MPPI::Config::field_goal_weight)
        .def_readwrite("field_cap", &MPPI::Config::field_cap)
        .def_readwrite("acceleration_limits", &MPPI::Config::acceleration_limits)
        .def_readwrite("footprint_margin", &MPPI::Config::footprint_margin);
    using Mover = Control::MovingObstacle;
    py::class_<Mover>(c, "MovingObstacle", "A disc that moves in a straight line: world metres and m/s at the time of the state")
        .def(py::init([](double x, double y, double vx, double vy, double radius) { return Mover{x, y, vx, vy, radius}; }),
             py::arg("x") = 0.0, py::arg("y") = 0.0, py::arg("vx") = 0.0, py::arg("vy") = 0.0, py::arg("radius") = 0.0)
        .def_readwrite("x", &Mover::x)
        .def_readwrite("y", &Mover::y)
        .def_readwrite("vx", &Mover::vx)
        .def_readwrite("vy", &Mover::vy)
        .def_readwrite("radius", &Mover::radius);
    auto movers_tuple = [](const MPPI::Movers &m) {
      return py::make_tuple(m.ox, m.oy, m.vx, m.vy, m.hq, m.sq, m.g, m.pen_hit, m.dropped);
    };
    py::class_<MPPI, Control::Follower>(c, "MPPI")
        .def(py::init<Control::ControlType, const Control::ControlLimitsParams &, double, const MPPI::Config &>(),
             py::arg("control_type"), py::arg("control_limits"), py::arg("time_step"), py::arg("config") = MPPI::Config())
        .def("execute", &MPPI::execute, py::arg("world_map"), py::arg("current_position"),
             "One MPPI step over the world map's distance plane: two launches and one read-back")
        .def("reset_sequence", &MPPI::resetSequence)
        .def("set_cost_field", &MPPI::setCostField, py::arg("planner"),
             "the planner's kept cost field in the place of the path, from the next execute() on (rules 19 to 24); the caller "
             "keeps the planner alive while it is attached")
        .def("clear_cost_field", &MPPI::clearCostField, "back to the path mode")
        .def_property_readonly("has_cost_field", &MPPI::hasCostField)
        .def("set_box_footprint", &MPPI::setBoxFootprint, py::arg("length"), py::arg("width"),
             "a box of length x width metres, the pose at its centre, covered by up to eight discs (rules 30 to 36), from the "
             "next execute() on")
        .def("clear_footprint", &MPPI::clearFootprint, "back to the one disc of hit_radius")
        .def_property_readonly("has_box_footprint", &MPPI::hasBoxFootprint)
        .def_property_readonly("field_at_robot", &MPPI::fieldAtRobot,
                               "f0 of the last step in field mode: the field at the robot's cell, 0xFFFFFFFF in an invalid or cut-off cell")
        .def_property_readonly("field_nominal", &MPPI::fieldNominal, "f_nom of the last step in field mode")
        .def("set_moving_obstacles", &MPPI::setMovingObstacles, py::arg("obstacles"),
             "the moving obstacles of the steps to come, at the time of the next step's state; kept until replaced or cleared")
        .def_property_readonly("moving_obstacles", &MPPI::movingObstacles)
        .def("set_follower_params", [](MPPI &m, const Control::Follower::FollowerParameters &p) { m.setParams(p); }, py::arg("params"),
             "the Follower's own parameters: goal tolerances, interpolation and segment lengths")
        .def("controls", &MPPI::controls, py::arg("n"), "the first n controls of the new sequence as (vx, vy, omega)")
        .def("predicted_path", &MPPI::predictedPath, "the new sequence rolled out on the host: (x, y, yaw) after each step")
        .def("sample_costs", &MPPI::sampleCosts)
        .def_property_readonly("last_sequence", &MPPI::lastSequence)
        .def_property_readonly("last_applied", &MPPI::lastApplied,
                               "with acceleration_limits, rule 28's applied sequence of the new one, T x 3 ints; empty otherwise")
        .def_property_readonly("last_velocity", &MPPI::lastVelocity,
                               "the applied (F, L, H) the last command was formed from: the next step's V0 (rule 28)")
        .def_property_readonly("last_record", [](const MPPI &m) {
               const kc_mppi_record &r = m.lastRecord();
               return py::make_tuple(r.s_min, r.k_best, r.s_0, r.den, r.n_hit, r.step);
             }, "(s_min, k_best, s_0, den, n_hit, step) of the last step")
        .def_property_readonly("last_n_hit_moving", [](const MPPI &m) { return m.lastRecord().n_hit_moving; },
                               "the samples among n_hit that a moving obstacle ended in the last step")
        .def_property_readonly("last_inputs", [movers_tuple](const MPPI &m) {
               const MPPI::Inputs &i = m.lastInputs();
               py::dict d;
               d["tx"] = i.tx;
               d["ty"] = i.ty;
               d["h"] = i.h;
               d["step"] = i.step;
               d["px"] = i.px;
               d["py"] = i.py;
               d["u"] = i.u;
               d["movers"] = movers_tuple(i.movers);
               d["field"] = i.field;
               d["limited"] = i.limited;
               d["rates"] = i.rates;
               d["v0"] = i.v0;
               d["offsets"] = i.offsets;
               d["r2"] = i.r2;
               return d;
             }, "the last step's inputs as the device took them")
        .def_static("quantise", [](Control::ControlType type, const Control::ControlLimitsParams &lim, double dt, float res,
                                   const MPPI::Config &cfg) {
               const MPPI::Quantised q = MPPI::quantise(type, lim, dt, res, cfg);
               return py::make_tuple(q.f_lo, q.f_hi, q.l_hi, q.h_hi, q.kq, q.s, q.rates);
             }, py::arg("control_type"), py::arg("control_limits"), py::arg("time_step"), py::arg("resolution"), py::arg("config"),
             "(F_lo, F_hi, L_hi, H_hi, kq, s[3], rates[6]): host only")
        .def_static("costs_of", [](const MPPI::Config &cfg) {
               const MPPI::Costs t = MPPI::costsOf(cfg);
               return py::make_tuple(t.r2, t.pen_d2, t.pen_far, t.pen_hit, t.w_path, t.qcap, t.w_goal, t.wtab, t.w_shift);
             }, py::arg("config"), "(r2, pen_d2, pen_far, pen_hit, w_path, qcap, w_goal, wtab, w_shift): host only")
        .def_static("movers_of", [movers_tuple](const std::vector<Mover> &obstacles, double dt, float res, double ox, double oy, double x,
                                                double y, const MPPI::Config &cfg, double hit_cells) {
               return movers_tuple(MPPI::moversOf(obstacles, dt, res, ox, oy, x, y, cfg, hit_cells));
             }, py::arg("obstacles"), py::arg("time_step"), py::arg("resolution"), py::arg("origin_x"), py::arg("origin_y"),
             py::arg("robot_x"), py::arg("robot_y"), py::arg("config"), py::arg("hit_cells") = -1.0,
             "(OX, OY, VX, VY, hq, sq, g, pen_hit_mv, dropped) against the origin given: host only; hit_cells >= 0 in the place "
             "of hit_radius (a box footprint's rho + margin)")
        .def_static("footprint_of", [](double length, double width, float res, double margin) {
               const MPPI::Footprint f = MPPI::footprintOf(length, width, res, margin);
               return py::make_tuple(f.offsets, f.r2, f.rho);
             }, py::arg("length"), py::arg("width"), py::arg("resolution"), py::arg("margin_cells") = 1.5,
             "rule 36: (offsets in 16 fraction bits of a cell, r2, rho in cells) of a box of length x width metres: host only")
        .def_static("from_tracked_box", [](const std::array<float, 3> &center, const std::array<float, 3> &size,
                                           const std::array<float, 3> &vel) {
               Bbox3D b;
               b.center = {center[0], center[1], center[2]};
               b.size = {size[0], size[1], size[2]};
               TrackedBbox3D t(b);
               t.vel = {vel[0], vel[1], vel[2]};
               return MPPI::fromTrackedBox(t);
             }, py::arg("center"), py::arg("size"), py::arg("vel"),
             "the MovingObstacle of a TrackedBbox3D that already lies in the world frame: centre, vel, hypot(size.x, size.y) / 2");
  }

  // PurePursuit (bindings_control.cpp:159-207)
  using PP = Control::PurePursuit;
  py::class_<PP::PurePursuitConfig, Control::Follower::FollowerParameters>(c, "PurePursuitConfig").def(py::init<>());
  py::class_<PP, Control::Follower>(c, "PurePursuit")
      .def(py::init([](const Control::ControlType &type, const Control::ControlLimitsParams &lim,
                       CollisionChecker::ShapeType shape, const std::vector<float> &dims, const py::object &spos,
                       const py::object &srot, double res, const PP::PurePursuitConfig &cfg) {
             return std::make_unique<PP>(type, lim, shape, dims, vec3(spos), vec4(srot), res, cfg);
           }), "Init PurePursuit follower with collision avoidance configuration", py::arg("control_type"),
           py::arg("control_limits"), py::arg("robot_shape_type"), py::arg("robot_dimensions"),
           py::arg("sensor_position_robot"), py::arg("sensor_rotation_robot"), py::arg("octree_res") = 0.1,
           py::arg("config") = PP::PurePursuitConfig())
      .def("execute", static_cast<Control::Controller::Result (PP::*)(const Path::State, const double)>(&PP::execute),
           "Execute Pure Pursuit control step with state update", py::arg("current_position"), py::arg("delta_time"))
      .def("execute", static_cast<Control::Controller::Result (PP::*)(const double)>(&PP::execute),
           "Execute Pure Pursuit control step (uses internal state)", py::arg("delta_time"))
      .def("execute", [](PP &self, const double dt, const Control::LaserScan &scan) {
             return self.execute<Control::LaserScan>(dt, scan);
           }, "Execute Pure Pursuit with LaserScan obstacle avoidance", py::arg("delta_time"), py::arg("laser_scan"))
      // (not in the reference: the obstacles of a WorldMap within sensor range, extracted on the device)
      .def("execute", [](PP &self, const double dt, const Mapping::WorldMap &map) {
             return self.execute<Mapping::WorldMap>(dt, map);
           }, "Execute Pure Pursuit with the obstacles of a world map", py::arg("delta_time"), py::arg("world_map"))
      .def("execute", [](PP &self, const double dt, const py::object &cloud) {
             // world-frame points: an (N, 3) float32 C-contiguous array is read where it lies, anything else
             // (lists of 3-sequences, other dtypes) is converted first
             const FArr a = py::cast<FArr>(cloud);
             if (a.ndim() != 2 || a.shape(1) != 3) throw std::invalid_argument("expected an (N, 3) array of points");
             return self.execute<Control::PointCloudView>(
                 dt, Control::PointCloudView{a.data(), static_cast<size_t>(a.shape(0))});
           }, "Execute Pure Pursuit with PointCloud obstacle avoidance", py::arg("delta_time"), py::arg("point_cloud"))
      // (not in the reference: the candidate list the avoidance search walks, nominal command first)
      .def("search_candidates", &PP::searchCandidates, py::arg("nominal"));

  // Vision followers (bindings_control.cpp:276-345)
  using RGB = Control::RGBFollower;
  py::class_<RGB::RGBFollowerConfig, Parameters>(c, "RGBFollowerParameters").def(py::init<>());
  c.attr("RGBFollowerConfig") = c.attr("RGBFollowerParameters");
  py::class_<RGB>(c, "RGBFollower")
      .def(py::init<const Control::ControlType, const Control::ControlLimitsParams, const RGB::RGBFollowerConfig>(),
           py::arg("control_type"), py::arg("control_limits"), py::arg("config") = RGB::RGBFollowerConfig())
      .def("reset_target", &RGB::resetTarget)
      .def("get_ctrl", &RGB::getCtrl)
      .def("get_errors", [](const RGB &f) { return arr(f.getErrors()); })
      .def("run", &RGB::run, py::arg("detection") = py::none())
      // (not in the reference: the queued search commands, front first)
      .def("pending_search_commands", &RGB::pendingSearchCommands);

  using RGBD = Control::RGBDFollower;
  py::class_<RGBD::RGBDFollowerConfig, RGB::RGBFollowerConfig>(c, "RGBDFollowerParameters").def(py::init<>());
  auto frame_call = [](RGBD &self, const DepthFrame &f, auto &&fn) {
    if (f.wait) self.depthAfterStream(f.stream);
    py::gil_scoped_release nogil;
    return fn();
  };
  py::class_<RGBD, Control::Follower>(c, "RGBDFollower")
      .def(py::init([](const Control::ControlType &type, const Control::ControlLimitsParams &lim,
                       const CollisionChecker::ShapeType &shape, const std::vector<float> &dims, const py::object &pos,
                       const py::object &rot, const RGBD::RGBDFollowerConfig &cfg) {
             return std::make_unique<RGBD>(type, lim, shape, dims, vec3(pos), vec4(rot), cfg);
           }), py::arg("control_type"), py::arg("control_limits"), py::arg("robot_shape_type"),
           py::arg("robot_dimensions"), py::arg("vision_sensor_position_wrt_body"),
           py::arg("vision_sensor_rotation_wrt_body"), py::arg("config") = RGBD::RGBDFollowerConfig())
      .def("set_camera_intrinsics", &RGBD::setCameraIntrinsics, py::arg("focal_length_x"), py::arg("focal_length_y"),
           py::arg("principal_point_x"), py::arg("principal_point_y"))
      .def("set_initial_tracking",
           py::overload_cast<const int, const int, const std::vector<Bbox3D> &, const float>(&RGBD::setInitialTracking),
           py::arg("pixel_x"), py::arg("pixel_y"), py::arg("detected_boxes_3d"), py::arg("robot_orientation") = 0.0)
      .def("set_initial_tracking",
           [frame_call](RGBD &self, int x, int y, const py::object &img, const std::vector<Bbox2D> &boxes, float yaw) {
             const DepthFrame f = depthFrame(img);
             return frame_call(self, f, [&] { return self.setInitialTracking(x, y, f.view, boxes, yaw); });
           }, py::arg("pixel_x"), py::arg("pixel_y"), py::arg("aligned_depth_image"), py::arg("detected_boxes_2d"),
           py::arg("robot_orientation") = 0.0)
      .def("set_initial_tracking",
           [frame_call](RGBD &self, const py::object &img, const Bbox2D &box, float yaw) {
             const DepthFrame f = depthFrame(img);
             return frame_call(self, f, [&] { return self.setInitialTracking(f.view, box, yaw); });
           }, py::arg("aligned_depth_image"), py::arg("target_box_2d"), py::arg("robot_orientation") = 0.0)
      .def("get_errors", [](const RGBD &f) { return arr(f.getErrors()); })
      .def("get_tracking_ctrl",
           py::overload_cast<const std::vector<Bbox3D> &, const Control::Velocity2D &>(&RGBD::getTrackingCtrl),
           py::arg("detected_boxes_3d"), py::arg("robot_velocity"))
      .def("get_tracking_ctrl",
           [frame_call](RGBD &self, const py::object &img, const std::vector<Bbox2D> &boxes,
                        const Control::Velocity2D &vel) {
             const DepthFrame f = depthFrame(img);
             return frame_call(self, f, [&] { return self.getTrackingCtrl(f.view, boxes, vel); });
           }, py::arg("aligned_depth_image"), py::arg("detected_boxes_2d"), py::arg("robot_velocity"))
      // (not in the reference: what the tests and tools read)
      .def("get_tracked_state", [](const RGBD &f) { return trackedState(f.getTrackedState()); },
           "The tracker's Kalman state (x, y, yaw, vx, vy, omega, ax, ay, a_yaw), or None")
      .def("get_raw_tracking", [](const RGBD &f) -> py::object {
             auto r = f.getRawTracking();
             return r ? py::cast(r->box) : py::none();
           }, "The last box the tracker accepted, or None")
      .def("pending_search_commands", &RGBD::pendingSearchCommands)
      .def("target_radius", &RGBD::targetRadius)
      .def("robot_radius", &RGBD::robotRadius)
      .def("goal_dist_tolerance", &RGBD::goalDistTolerance)
      .def("depth_calls", &RGBD::depthCalls)
      .def("depth_last_upload", &RGBD::depthLastUpload);

  // -------------------------------------------------------------- mapping
  auto mp = m.def_submodule("mapping", "Local Mapping module");
  py::enum_<Mapping::OccupancyType>(mp, "OCCUPANCY_TYPE")
      .value("UNEXPLORED", Mapping::OccupancyType::UNEXPLORED)
      .value("EMPTY", Mapping::OccupancyType::EMPTY)
      .value("OCCUPIED", Mapping::OccupancyType::OCCUPIED);

  auto gridView = [](Eigen::MatrixXi &g, py::handle owner) {
    // column-major (H, W) view into the mapper's member matrix, like
    // nanobind's reference_internal on an Eigen::MatrixXi
    return py::array_t<int>({(py::ssize_t)g.rows(), (py::ssize_t)g.cols()},
                            {(py::ssize_t)sizeof(int), (py::ssize_t)(sizeof(int) * g.rows())}, g.data(), owner);
  };

  auto probView = [](Eigen::MatrixXf &g, py::handle owner) {
    return py::array_t<float>({(py::ssize_t)g.rows(), (py::ssize_t)g.cols()},
                              {(py::ssize_t)sizeof(float), (py::ssize_t)(sizeof(float) * g.rows())}, g.data(),
                              owner);
  };

  py::class_<Mapping::LocalMapper>(mp, "LocalMapper")
      .def(py::init([](int H, int W, float res, const py::object &pos, float orient, bool pc, int scan, float step,
                       float maxh, float minh, float rmax, int mppl, int threads) {
             return std::make_unique<Mapping::LocalMapper>(H, W, res, vec3(pos), orient, pc, scan, step, maxh, minh, rmax, mppl, threads);
           }), py::arg("grid_height"), py::arg("grid_width"), py::arg("resolution"), py::arg("laserscan_position"),
           py::arg("laserscan_orientation"), py::arg("is_pointcloud"), py::arg("scan_size"), py::arg("angle_step"),
           py::arg("max_height"), py::arg("min_height"), py::arg("range_max"), py::arg("max_points_per_line") = 32,
           py::arg("max_num_threads") = 1)
      .def(py::init([](int H, int W, float res, const py::object &pos, float orient, bool pc, int scan, float pp,
                       float po, float pe, float rs, float rmax, float wall, float step, float maxh, float minh,
                       int mppl, int threads) {
             return std::make_unique<Mapping::LocalMapper>(H, W, res, vec3(pos), orient, pc, scan, pp, po, pe, rs, rmax, wall, step, maxh, minh, mppl, threads);
           }), py::arg("grid_height"), py::arg("grid_width"), py::arg("resolution"), py::arg("laserscan_position"),
           py::arg("laserscan_orientation"), py::arg("is_pointcloud"), py::arg("scan_size"), py::arg("p_prior"),
           py::arg("p_occupied"), py::arg("p_empty"), py::arg("range_sure"), py::arg("range_max"), py::arg("wall_size"),
           py::arg("angle_step"), py::arg("max_height"), py::arg("min_height"), py::arg("max_points_per_line"),
           py::arg("max_num_threads") = 1)
      .def("scan_to_grid", [gridView](py::object self, const DArr &angles, const DArr &ranges) {
             return gridView(self.cast<Mapping::LocalMapper &>().scanToGrid(dvec(angles), dvec(ranges)), self);
           }, "Convert laser scan data to occupancy grid (float64 arrays: one copy each)", py::arg("angles").noconvert(),
           py::arg("ranges").noconvert())
      .def("scan_to_grid", [gridView](py::object self, const std::vector<double> &angles, const std::vector<double> &ranges) {
             return gridView(self.cast<Mapping::LocalMapper &>().scanToGrid(angles, ranges), self);
           }, "Convert laser scan data to occupancy grid", py::arg("angles"), py::arg("ranges"))
      .def("scan_to_grid_on_device", [](Mapping::LocalMapper &m, const DArr &angles, const DArr &ranges) {
             m.scanToGridOnDevice(dvec(angles), dvec(ranges));
           }, "Scan into the device-resident grid only (float64 arrays: one copy each)", py::arg("angles").noconvert(),
           py::arg("ranges").noconvert())
      .def("scan_to_grid_on_device", &Mapping::LocalMapper::scanToGridOnDevice,
           "Scan into the device-resident grid only (for DWA.compute_velocity_commands(vel, mapper))",
           py::arg("angles"), py::arg("ranges"))
      .def("scan_to_grid", [gridView](py::object self, const std::vector<int8_t> &data, int point_step, int row_step,
                                      int height, int width, float x_offset, float y_offset, float z_offset) {
             return gridView(self.cast<Mapping::LocalMapper &>().scanToGrid(data, point_step, row_step, height, width,
                                                                           x_offset, y_offset, z_offset), self);
           }, "Convert a raw point cloud to occupancy grid", py::arg("data"), py::arg("point_step"),
           py::arg("row_step"), py::arg("height"), py::arg("width"), py::arg("x_offset"), py::arg("y_offset"),
           py::arg("z_offset"))
      // The reference binds scan_to_grid_baysian to scanToGrid
      // (bindings_mapping.cpp:59-75) while its own Python caller unpacks two
      // grids (mapping/local_mapper.py:289-306): bound here to the real
      // scanToGridBaysian, which is what that caller needs.
      .def("scan_to_grid_baysian", [gridView, probView](py::object self, const DArr &angles, const DArr &ranges) {
             auto r = self.cast<Mapping::LocalMapper &>().scanToGridBaysian(dvec(angles), dvec(ranges));
             return py::make_tuple(gridView(std::get<0>(r), self), probView(std::get<1>(r), self));
           }, "Convert laser scan data to occupancy grid, with baysian update (float64 arrays: one copy each)",
           py::arg("angles").noconvert(), py::arg("ranges").noconvert())
      .def("scan_to_grid_baysian", [gridView, probView](py::object self, const std::vector<double> &angles,
                                                        const std::vector<double> &ranges) {
             auto r = self.cast<Mapping::LocalMapper &>().scanToGridBaysian(angles, ranges);
             return py::make_tuple(gridView(std::get<0>(r), self), probView(std::get<1>(r), self));
           }, "Convert laser scan data to occupancy grid, with baysian update", py::arg("angles"), py::arg("ranges"))
      .def("scan_to_grid_baysian", [gridView, probView](py::object self, const std::vector<int8_t> &data,
                                                        int point_step, int row_step, int height, int width,
                                                        float x_offset, float y_offset, float z_offset) {
             auto r = self.cast<Mapping::LocalMapper &>().scanToGridBaysian(data, point_step, row_step, height,
                                                                            width, x_offset, y_offset, z_offset);
             return py::make_tuple(gridView(std::get<0>(r), self), probView(std::get<1>(r), self));
           }, "Convert a raw point cloud to occupancy grid, with baysian update", py::arg("data"),
           py::arg("point_step"), py::arg("row_step"), py::arg("height"), py::arg("width"), py::arg("x_offset"),
           py::arg("y_offset"), py::arg("z_offset"))
      // returns the warped grid (the reference returns None and its Python
      // caller stores the result; `unknown_value`, which that caller passes, is
      // accepted and unused: the fill value is the mapper's p_prior,
      // local_mapper.cpp:41)
      .def("get_previous_grid_in_current_pose", [probView](py::object self, const py::object &pos, double orient,
                                                           const py::object &) {
             auto &m = self.cast<Mapping::LocalMapper &>();
             auto v = py::cast<std::vector<float>>(pos);
             if (v.size() < 2) throw std::invalid_argument("current_position_in_previous_pose needs x and y");
             m.getPreviousGridInCurrentPose(Eigen::Vector2f(v[0], v[1]), orient);
             return probView(m.previousGridProb(), self);
           }, py::arg("current_position_in_previous_pose"), py::arg("current_orientation_in_previous_pose"),
           py::arg("unknown_value") = py::none())
      .def("set_previous_grid", [](Mapping::LocalMapper &m, const py::object &prob) {
             if (prob.is_none()) {
               m.setPreviousGridProb(nullptr);
               return;
             }
             auto a = py::array_t<float, py::array::f_style | py::array::forcecast>::ensure(prob);
             if (!a || a.ndim() != 2) throw std::invalid_argument("previous grid must be a 2-D array");
             Eigen::MatrixXf g(static_cast<int>(a.shape(0)), static_cast<int>(a.shape(1)));
             std::memcpy(g.data(), a.data(), sizeof(float) * static_cast<size_t>(a.size()));
             m.setPreviousGridProb(&g);
           }, "Replace the previous probability grid (None: feed the last scan's probabilities back)",
           py::arg("previous_grid") = py::none());

  py::class_<Mapping::LocalMapperGPU, Mapping::LocalMapper>(mp, "LocalMapperGPU")
      .def(py::init([](int H, int W, float res, const py::object &pos, float orient, bool pc, int scan, float step,
                       float maxh, float minh, float rmax, int mppl) {
             return std::make_unique<Mapping::LocalMapperGPU>(H, W, res, vec3(pos), orient, pc, scan, step, maxh, minh, rmax, mppl);
           }), py::arg("grid_height"), py::arg("grid_width"), py::arg("resolution"), py::arg("laserscan_position"),
           py::arg("laserscan_orientation"), py::arg("is_pointcloud"), py::arg("scan_size"), py::arg("angle_step"),
           py::arg("max_height"), py::arg("min_height"), py::arg("range_max"), py::arg("max_points_per_line") = 32);

  // not in the reference, which leaves the world-frame map to its ROS side
  py::class_<WorldMapDeviceGrid>(mp, "WorldMapDeviceGrid")
      .def_property_readonly("__cuda_array_interface__", &worldMapInterface)
      .def_property_readonly("shape", [](const WorldMapDeviceGrid &g) { return py::make_tuple(g.width, g.height); });
  auto plane = [](const std::vector<int8_t> &v, int w, int h) {
    py::array_t<int8_t, py::array::f_style> a({(py::ssize_t)w, (py::ssize_t)h});
    if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size());
    return a;
  };
  py::class_<WorldMapMatch>(mp, "WorldMapMatch")
      .def_property_readonly("k", [](const WorldMapMatch &r) { return r.m.k; })
      .def_property_readonly("u", [](const WorldMapMatch &r) { return r.m.u; })
      .def_property_readonly("v", [](const WorldMapMatch &r) { return r.m.v; })
      .def_property_readonly("score", [](const WorldMapMatch &r) { return r.m.score; })
      .def_property_readonly("score_guess", [](const WorldMapMatch &r) { return r.m.score_guess; })
      .def_property_readonly("points", [](const WorldMapMatch &r) { return r.m.points; })
      .def_property_readonly("x", [](const WorldMapMatch &r) { return r.m.x; })
      .def_property_readonly("y", [](const WorldMapMatch &r) { return r.m.y; })
      .def_property_readonly("yaw", [](const WorldMapMatch &r) { return r.m.yaw; })
      .def_property_readonly("pose", [](const WorldMapMatch &r) {
             return py::make_tuple(r.m.pose.cq, r.m.pose.sq, r.m.pose.tx, r.m.pose.ty);
           }, "the corrected pose as the update takes it: (cq, sq, tx, ty), 16 fraction bits")
      .def("scores", &worldMapMatchScores,
           "the score table, uint32 [2 n_yaw + 1, 2 reach + 1, 2 reach + 1] indexed [k + n_yaw, v + reach, u + reach]; "
           "RuntimeError once the map has made another match");
  py::class_<Mapping::MoverDetectConfig>(mp, "MoverDetectConfig",
                                         "WorldMap.detect_movers' parameters (DESIGN.md 4.11 rule 64); the defaults are judgement")
      .def(py::init([](uint32_t m2, uint32_t gap, uint64_t join_q, uint32_t min_beams) {
             Mapping::MoverDetectConfig c;
             c.m2 = m2, c.gap = gap, c.join_q = join_q, c.min_beams = min_beams;
             return c;
           }), py::arg("m2") = 4, py::arg("gap") = 2, py::arg("join_q") = 9ull << 16, py::arg("min_beams") = 3)
      .def_readwrite("m2", &Mapping::MoverDetectConfig::m2)
      .def_readwrite("gap", &Mapping::MoverDetectConfig::gap)
      .def_readwrite("join_q", &Mapping::MoverDetectConfig::join_q)
      .def_readwrite("min_beams", &Mapping::MoverDetectConfig::min_beams);
  py::class_<Mapping::MoverCluster>(mp, "MoverCluster", "A kept cluster: world metres, and rule 68's integers")
      .def(py::init([](double x, double y, double radius) {
             Mapping::MoverCluster c;
             c.x = x, c.y = y, c.radius = radius;
             return c;
           }), py::arg("x") = 0.0, py::arg("y") = 0.0, py::arg("radius") = 0.0)
      .def_readwrite("x", &Mapping::MoverCluster::x)
      .def_readwrite("y", &Mapping::MoverCluster::y)
      .def_readwrite("radius", &Mapping::MoverCluster::radius)
      .def_property_readonly("raw", [](const Mapping::MoverCluster &c) {
             const kc_worldmap_cluster &r = c.raw;
             return py::make_tuple(r.k_first, r.k_last, r.n, r.sx, r.sy, r.min_x, r.max_x, r.min_y, r.max_y);
           }, "(k_first, k_last, n, sx, sy, min_x, max_x, min_y, max_y)");
  py::class_<Mapping::MoverDetection>(mp, "MoverDetection")
      .def_readonly("clusters", &Mapping::MoverDetection::clusters)
      .def_property_readonly("labels", [](const Mapping::MoverDetection &d) {
             return py::array_t<int32_t>(static_cast<py::ssize_t>(d.labels.size()), d.labels.data());
           }, "int32 a beam: the kept cluster's number, -1 not dynamic, -2 a dynamic beam of a dropped run")
      .def_property_readonly("record", [](const Mapping::MoverDetection &d) {
             return py::make_tuple(d.record.n_dynamic, d.record.n_runs, d.record.n_kept, d.record.n_returned);
           }, "(n_dynamic, n_runs, n_kept, n_returned)");
  {
    using Tracker = Mapping::MoverTracker;
    py::class_<Tracker::Track>(mp, "MoverTrack")
        .def_readonly("id", &Tracker::Track::id)
        .def_readonly("x", &Tracker::Track::x)
        .def_readonly("y", &Tracker::Track::y)
        .def_readonly("vx", &Tracker::Track::vx)
        .def_readonly("vy", &Tracker::Track::vy)
        .def_readonly("radius", &Tracker::Track::radius)
        .def_readonly("hits", &Tracker::Track::hits)
        .def_readonly("misses", &Tracker::Track::misses);
    py::class_<Tracker>(mp, "MoverTracker",
                        "Alpha-beta tracks over detect_movers' clusters, greedy nearest neighbour; host only.  The defaults are judgement")
        .def(py::init([](double alpha, double beta, int max_misses, double gate) {
               Mapping::MoverTrackerConfig c;
               c.alpha = alpha, c.beta = beta, c.max_misses = max_misses, c.gate = gate;
               return std::make_unique<Tracker>(c);
             }), py::arg("alpha") = 0.5, py::arg("beta") = 0.3, py::arg("max_misses") = 3, py::arg("gate") = 6.0)
        .def("update", [](Tracker &t, const std::vector<Mapping::MoverCluster> &clusters, double dt) { t.update(clusters, dt); },
             py::arg("clusters"), py::arg("dt"))
        .def("update", [](Tracker &t, const Mapping::MoverDetection &d, double dt) { t.update(d, dt); }, py::arg("detection"),
             py::arg("dt"))
        .def_property_readonly("tracks", &Tracker::tracks)
        .def("moving_obstacles", &Tracker::movingObstacles, "a MovingObstacle for every live track")
        .def_static("skip_mask", [](const std::vector<int32_t> &labels) {
               const std::vector<uint8_t> m = Tracker::skipMask(labels);
               return py::array_t<uint8_t>(static_cast<py::ssize_t>(m.size()), m.data());
             }, py::arg("labels"), "uint8 a beam: 1 for the member beams of every kept cluster")
        .def("clear", &Tracker::clear);
  }
  py::class_<Mapping::WorldMap>(mp, "WorldMap")
      .def(py::init([](int width, int height, float resolution, double origin_x, double origin_y) {
             return std::make_unique<Mapping::WorldMap>(width, height, resolution, origin_x, origin_y);
           }), py::arg("width"), py::arg("height"), py::arg("resolution"), py::arg("origin_x") = 0.0, py::arg("origin_y") = 0.0)
      .def("set_model", &Mapping::WorldMap::setModel, py::arg("hit") = 3, py::arg("miss") = 1, py::arg("e_min") = -8,
           py::arg("e_max") = 14, py::arg("occ_thr") = 1,
           "Evidence an OCCUPIED / EMPTY observation adds / takes away within e_min .. e_max, OCCUPIED from occ_thr up; clears the map")
      .def("set_prior", &worldMapSetPrior, py::arg("grid"),
           "A (width, height) int32 / int8 grid replaces the state: a numpy array, or a device array read in place")
      .def("update", [](Mapping::WorldMap &m, const Mapping::LocalMapper &mapper, double x, double y, double yaw) {
             py::gil_scoped_release nogil;
             return m.update(mapper, x, y, yaw);
           }, py::arg("mapper"), py::arg("x"), py::arg("y"), py::arg("yaw"),
           "Fuse the mapper's last grid where it lies on the device; (x, y, yaw): the robot's pose in the world.  -> changed cells")
      .def("update", [](Mapping::WorldMap &m, const py::array &grid, double x, double y, double yaw) {
             const auto g = worldMapLocalGrid(grid);
             const int32_t *d = g.data();
             const int gh = static_cast<int>(g.shape(0)), gw = static_cast<int>(g.shape(1));
             py::gil_scoped_release nogil;
             return m.update(d, gh, gw, x, y, yaw);
           }, py::arg("grid"), py::arg("x"), py::arg("y"), py::arg("yaw"),
           "Fuse a (grid_height, grid_width) int32 grid from the host, the mapper's central cell.  -> changed cells")
      .def("match", [](py::object self, const Mapping::LocalMapper &mapper, double x, double y, double yaw, int n_yaw,
                       double yaw_step, int reach) {
             auto &m = self.cast<Mapping::WorldMap &>();
             Mapping::WorldMap::Match r;
             {
               py::gil_scoped_release nogil;
               r = m.match(mapper, x, y, yaw, n_yaw, yaw_step, reach);
             }
             return WorldMapMatch{r, self, m.matchCount()};
           }, py::arg("local"), py::arg("x"), py::arg("y"), py::arg("yaw"), py::arg("n_yaw"), py::arg("yaw_step"), py::arg("reach"),
           "Match the mapper's last grid where it lies against the map around the guess (x, y, yaw); the map is not modified")
      .def("match", [](py::object self, const py::array &grid, double x, double y, double yaw, int n_yaw, double yaw_step,
                       int reach) {
             auto &m = self.cast<Mapping::WorldMap &>();
             const auto g = worldMapLocalGrid(grid);
             const int32_t *d = g.data();
             const int gh = static_cast<int>(g.shape(0)), gw = static_cast<int>(g.shape(1));
             Mapping::WorldMap::Match r;
             {
               py::gil_scoped_release nogil;
               r = m.match(d, gh, gw, x, y, yaw, n_yaw, yaw_step, reach);
             }
             return WorldMapMatch{r, self, m.matchCount()};
           }, py::arg("local"), py::arg("x"), py::arg("y"), py::arg("yaw"), py::arg("n_yaw"), py::arg("yaw_step"), py::arg("reach"),
           "Match a (grid_height, grid_width) int32 grid from the host, the mapper's central cell")
      .def("update_at", [](Mapping::WorldMap &m, const Mapping::LocalMapper &mapper, const py::tuple &pose) {
             const kc_worldmap_pose p = worldMapPose(pose);
             py::gil_scoped_release nogil;
             return m.updateAt(mapper, p);
           }, py::arg("mapper"), py::arg("pose"), "update at a quantised pose (cq, sq, tx, ty), a match's `pose`")
      .def("update_at", [](Mapping::WorldMap &m, const py::array &grid, const py::tuple &pose) {
             const kc_worldmap_pose p = worldMapPose(pose);
             const auto g = worldMapLocalGrid(grid);
             const int32_t *d = g.data();
             const int gh = static_cast<int>(g.shape(0)), gw = static_cast<int>(g.shape(1));
             py::gil_scoped_release nogil;
             return m.updateAt(d, gh, gw, p);
           }, py::arg("grid"), py::arg("pose"), "update at a quantised pose (cq, sq, tx, ty), a match's `pose`")
      .def("clear", &Mapping::WorldMap::clear)
      .def("points", [](const Mapping::WorldMap &m, double x, double y, float max_sensor_range) {
             std::vector<Path::Point> pts;
             {
               py::gil_scoped_release nogil;
               pts = m.points(x, y, max_sensor_range);
             }
             FArr a({(py::ssize_t)pts.size(), (py::ssize_t)3});
             if (!pts.empty()) std::memcpy(a.mutable_data(), pts.data()->data(), sizeof(float) * 3 * pts.size());
             return a;
           }, py::arg("x"), py::arg("y"), py::arg("max_sensor_range"),
           "The occupied cells within max_sensor_range of (x, y) as world-frame points, float32 [n, 3], in no particular order")
      .def("scan", [](const Mapping::WorldMap &m, double x, double y, double yaw, const std::vector<double> &angles,
                      float range_max, bool unknown_blocks, bool return_cells) -> py::object {
             std::vector<double> r;
             std::vector<int32_t> c;
             {
               py::gil_scoped_release nogil;
               r = return_cells ? m.scanCells(x, y, yaw, angles, range_max, unknown_blocks, c)
                                : m.scan(x, y, yaw, angles, range_max, unknown_blocks);
             }
             py::array_t<double> ra(static_cast<py::ssize_t>(r.size()), r.data());
             if (!return_cells) return std::move(ra);
             return py::make_tuple(ra, py::array_t<int32_t>(static_cast<py::ssize_t>(c.size()), c.data()));
           }, py::arg("x"), py::arg("y"), py::arg("yaw"), py::arg("angles"), py::arg("range_max"),
           py::arg("unknown_blocks") = false, py::arg("return_cells") = false,
           "The map's virtual laser scan from the frame (x, y, yaw): float64 [B], the distance to the first occupied cell "
           "along every beam angle within range_max, else range_max; with return_cells also the hit cells I + J * width")
      .def("scans", [](const Mapping::WorldMap &m, const std::vector<std::array<double, 3>> &poses,
                       const std::vector<double> &angles, float range_max, bool unknown_blocks) {
             std::vector<double> r;
             {
               py::gil_scoped_release nogil;
               r = m.scans(poses, angles, range_max, unknown_blocks);
             }
             py::array_t<double> a({static_cast<py::ssize_t>(poses.size()), static_cast<py::ssize_t>(angles.size())});
             if (!r.empty()) std::memcpy(a.mutable_data(), r.data(), sizeof(double) * r.size());
             return a;
           }, py::arg("poses"), py::arg("angles"), py::arg("range_max"), py::arg("unknown_blocks") = false,
           "The same for a batch of poses (x, y, yaw) in one launch: float64 [M, B]")
      .def("integrate_scan", [](Mapping::WorldMap &m, double x, double y, double yaw, const std::vector<double> &angles,
                                const std::vector<double> &ranges, float range_max, float range_min, bool clear_no_return,
                                const std::vector<uint8_t> &skip) {
             py::gil_scoped_release nogil;
             return m.integrateScan(x, y, yaw, angles, ranges, range_max, range_min, clear_no_return, skip);
           }, py::arg("x"), py::arg("y"), py::arg("yaw"), py::arg("angles"), py::arg("ranges"), py::arg("range_max"),
           py::arg("range_min") = 0.0f, py::arg("clear_no_return") = false, py::arg("skip") = std::vector<uint8_t>(),
           "One measured laser scan into the map by an inverse ray cast (DESIGN.md 4.11 rules 52 to 58); (x, y, yaw): the scan "
           "frame's pose in the world; skip: empty, or an entry a beam, not 0 where the beam is to say nothing.  -> changed cells")
      .def("integrate_scan_at", [](Mapping::WorldMap &m, const py::tuple &pose, const std::vector<double> &angles,
                                   const std::vector<double> &ranges, float range_max, float range_min, bool clear_no_return,
                                   const std::vector<uint8_t> &skip) {
             const kc_worldmap_pose p = worldMapPose(pose);
             py::gil_scoped_release nogil;
             return m.integrateScanAt(p, angles, ranges, range_max, range_min, clear_no_return, skip);
           }, py::arg("pose"), py::arg("angles"), py::arg("ranges"), py::arg("range_max"), py::arg("range_min") = 0.0f,
           py::arg("clear_no_return") = false, py::arg("skip") = std::vector<uint8_t>(),
           "integrate_scan at a quantised pose (cq, sq, tx, ty), a match's `pose`")
      .def("detect_movers", [](const Mapping::WorldMap &m, double x, double y, double yaw, const std::vector<double> &angles,
                               const std::vector<double> &ranges, float range_max, float range_min,
                               const Mapping::MoverDetectConfig &config) {
             py::gil_scoped_release nogil;
             return m.detectMovers(x, y, yaw, angles, ranges, range_max, range_min, config);
           }, py::arg("x"), py::arg("y"), py::arg("yaw"), py::arg("angles"), py::arg("ranges"), py::arg("range_max"),
           py::arg("range_min") = 0.0f, py::arg("config") = Mapping::MoverDetectConfig(),
           "Moving obstacles in a measured scan (DESIGN.md 4.11 rules 64 to 69): the returns that end in free space the map has "
           "seen, grouped into clusters in world metres, and a label a beam.  The distance plane must be on.  -> MoverDetection")
      .def("detect_movers_at", [](const Mapping::WorldMap &m, const py::tuple &pose, const std::vector<double> &angles,
                                  const std::vector<double> &ranges, float range_max, float range_min,
                                  const Mapping::MoverDetectConfig &config) {
             const kc_worldmap_pose p = worldMapPose(pose);
             py::gil_scoped_release nogil;
             return m.detectMoversAt(p, angles, ranges, range_max, range_min, config);
           }, py::arg("pose"), py::arg("angles"), py::arg("ranges"), py::arg("range_max"), py::arg("range_min") = 0.0f,
           py::arg("config") = Mapping::MoverDetectConfig(), "detect_movers at a quantised pose (cq, sq, tx, ty)")
      .def_static("cluster_to_world", [](const py::tuple &raw, float resolution, double origin_x, double origin_y) {
             if (raw.size() != 9) throw std::invalid_argument("a raw cluster has nine entries");
             kc_worldmap_cluster c{};
             c.k_first = raw[0].cast<int32_t>(), c.k_last = raw[1].cast<int32_t>(), c.n = raw[2].cast<int32_t>();
             c.sx = raw[3].cast<int64_t>(), c.sy = raw[4].cast<int64_t>();
             c.min_x = raw[5].cast<int64_t>(), c.max_x = raw[6].cast<int64_t>();
             c.min_y = raw[7].cast<int64_t>(), c.max_y = raw[8].cast<int64_t>();
             return Mapping::WorldMap::clusterToWorld(c, resolution, origin_x, origin_y);
           }, py::arg("raw"), py::arg("resolution"), py::arg("origin_x"), py::arg("origin_y"),
           "A cluster's (k_first, k_last, n, sx, sy, min_x, max_x, min_y, max_y) in world metres; needs no device")
      .def("enable_distance", &Mapping::WorldMap::enableDistance, py::arg("reach"), py::arg("unknown_blocks") = false,
           "Keep the distance plane at `reach` cells (1 .. 254; 0: off): DESIGN.md 4.11 rules 42 and 43")
      .def_property_readonly("distance_reach", &Mapping::WorldMap::distanceReach)
      .def("distance_field", [](const Mapping::WorldMap &m) {
             const std::vector<uint16_t> v = m.distanceField();
             py::array_t<uint16_t, py::array::f_style> a({static_cast<py::ssize_t>(m.width()), static_cast<py::ssize_t>(m.height())});
             std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(uint16_t));
             return a;
           }, "the refreshed distance plane, uint16 [width, height]: squared cells to the nearest blocking cell, 0xFFFF beyond reach")
      .def("distance_last_box", [](const Mapping::WorldMap &m) {
             const auto b = m.distanceLastBox();
             return py::make_tuple(b[0], b[1], b[2], b[3]);
           }, "(i_min, j_min, i_max, j_max) the last refresh recomputed; all -1 when it had nothing to do")
      .def("device_distance_ptr", [](const Mapping::WorldMap &m) { return reinterpret_cast<uintptr_t>(m.deviceDistance()); },
           "the refreshed plane's device address: uint16, (width, height), column-major")
      .def("get_cls", [plane](const Mapping::WorldMap &m) { return plane(m.cls(), m.width(), m.height()); },
           "the class plane, int8 [width, height]: -1 unexplored, 0 empty, 100 occupied")
      .def("get_evidence", [plane](const Mapping::WorldMap &m) { return plane(m.evidence(), m.width(), m.height()); },
           "the evidence plane, int8 [width, height]: -128 never observed")
      .def("get_changed", &Mapping::WorldMap::changed, "cells whose class the last update changed")
      .def("get_changed_box", [](const Mapping::WorldMap &m) {
             const auto b = m.changedBox();
             return py::make_tuple(b[0], b[1], b[2], b[3]);
           }, "(i_min, j_min, i_max, j_max) of those cells; all -1 when there are none")
      .def("device_grid", [](py::object self) {
             const auto &m = self.cast<const Mapping::WorldMap &>();
             return WorldMapDeviceGrid{self, static_cast<uint64_t>(reinterpret_cast<uintptr_t>(m.deviceGrid())), m.width(), m.height()};
           }, "The class plane on the device: an object with __cuda_array_interface__ that GridPlanner.set_grid reads in place")
      .def_static("quantise_pose", [](float resolution, double origin_x, double origin_y, double x, double y, double yaw) {
             const kc_worldmap_pose p = Mapping::WorldMap::quantisePose(resolution, origin_x, origin_y, x, y, yaw);
             return py::make_tuple(p.cq, p.sq, p.tx, p.ty);
           }, py::arg("resolution"), py::arg("origin_x"), py::arg("origin_y"), py::arg("x"), py::arg("y"), py::arg("yaw"),
           "(cq, sq, tx, ty): the pose as the update takes it, 16 fraction bits; needs no device")
      .def("shift", [](Mapping::WorldMap &m, int di, int dj) {
             py::gil_scoped_release nogil;
             m.shift(di, dj);
           }, py::arg("di"), py::arg("dj"),
           "Move the window by whole cells on the device (DESIGN.md 4.11 rules 46 to 48), a positive di towards +x")
      .def("recentre", [](Mapping::WorldMap &m, double x, double y, int margin, int stride) {
             std::array<int, 2> d;
             {
               py::gil_scoped_release nogil;
               d = m.recentre(x, y, margin, stride);
             }
             return py::make_tuple(d[0], d[1]);
           }, py::arg("x"), py::arg("y"), py::arg("margin"), py::arg("stride"),
           "Rule 49's plan for the robot at world (x, y), then the shift -> (di, dj), the shift made")
      .def("offset", [](const Mapping::WorldMap &m) {
             const auto o = m.offset();
             return py::make_tuple(o[0], o[1]);
           }, "(OI, OJ): the cells the window has moved since it was created")
      .def_static("recentre_plan", [](int width, int height, int ic, int jc, int margin, int stride) {
             const auto d = Mapping::WorldMap::recentrePlan(width, height, ic, jc, margin, stride);
             return py::make_tuple(d[0], d[1]);
           }, py::arg("width"), py::arg("height"), py::arg("ic"), py::arg("jc"), py::arg("margin"), py::arg("stride"),
           "Rule 49 alone: the shift for a robot in cell (ic, jc); needs no device")
      .def_property_readonly("width", &Mapping::WorldMap::width)
      .def_property_readonly("height", &Mapping::WorldMap::height)
      .def_property_readonly("resolution", &Mapping::WorldMap::resolution)
      .def_property_readonly("origin", [](const Mapping::WorldMap &m) { return py::make_tuple(m.originX(), m.originY()); },
                             "the world position of cell (0, 0)'s centre at the current offset");

  // (not in the reference: Monte-Carlo localisation over a WorldMap, the particles on the device; DESIGN.md 4.11 rules
  // 28 to 41)
  {
    using MCL = Mapping::MCL;
    // SX, SY as Python ints: (hi << 64) + lo
    auto wideInt = [](uint64_t lo, int64_t hi) { return (py::int_(hi) << py::int_(64)) + py::int_(lo); };
    py::class_<MCL::Estimate>(mp, "MCLEstimate")
        .def_readonly("x", &MCL::Estimate::x)
        .def_readonly("y", &MCL::Estimate::y)
        .def_readonly("yaw", &MCL::Estimate::yaw)
        .def_readonly("n_eff", &MCL::Estimate::n_eff)
        .def_readonly("spread", &MCL::Estimate::spread)
        .def_readonly("resampled", &MCL::Estimate::resampled)
        .def_readonly("best_cost", &MCL::Estimate::best_cost)
        .def_readonly("txe", &MCL::Estimate::txe)
        .def_readonly("tye", &MCL::Estimate::tye)
        .def_readonly("fit", &MCL::Estimate::fit, "the step's mean penalty a contributing beam in 1 / 256 (rule 60), -1 without one")
        .def_readonly("fit_slow", &MCL::Estimate::fit_slow)
        .def_readonly("fit_fast", &MCL::Estimate::fit_fast)
        .def_readonly("injected", &MCL::Estimate::injected, "the slots the step's resample drew anew over the free cells")
        .def_readonly("cost_min", &MCL::Estimate::cost_min)
        .def_readonly("cost_best", &MCL::Estimate::cost_best)
        .def_readonly("beams_used", &MCL::Estimate::beams_used)
        .def_property_readonly("record", [wideInt](const MCL::Estimate &e) {
               const kc_mcl_record &r = e.record;
               return py::make_tuple(r.w1, r.w2, wideInt(r.sx_lo, r.sx_hi), wideInt(r.sy_lo, r.sy_hi), r.sc, r.ss, r.amin, r.best,
                                     r.best_tx, r.best_ty, r.best_h, r.step);
             }, "(w1, w2, sx, sy, sc, ss, amin, best, best_tx, best_ty, best_h, step): rule 37's exact sums");
    py::class_<MCL>(mp, "MCL")
        .def(py::init([](const Mapping::WorldMap &map, size_t n_particles, const std::vector<double> &angles, float range_max,
                         uint64_t seed) { return std::make_unique<MCL>(map, n_particles, angles, range_max, seed); }),
             py::arg("world_map"), py::arg("n_particles"), py::arg("angles"), py::arg("range_max"), py::arg("seed") = 0,
             py::keep_alive<1, 2>())
        .def("set_model", [](MCL &m, double sigma_hit, int err_shift, int n_pen, double floor, double pen_scale, int w_shift, int n_w,
                             uint32_t wtab0, double temperature) {
               MCL::Model d;
               d.sigma_hit = sigma_hit;
               d.err_shift = err_shift;
               d.n_pen = n_pen;
               d.floor = floor;
               d.pen_scale = pen_scale;
               d.w_shift = w_shift;
               d.n_w = n_w;
               d.wtab0 = wtab0;
               d.temperature = temperature;
               m.setModel(d);
             }, py::arg("sigma_hit") = 0.1, py::arg("err_shift") = 12, py::arg("n_pen") = 256, py::arg("floor") = 0.05,
             py::arg("pen_scale") = 64.0, py::arg("w_shift") = 4, py::arg("n_w") = 1024, py::arg("wtab0") = 1u << 16,
             py::arg("temperature") = 256.0, "The sensor model the penalty and weight tables are built from (judgement)")
        .def("set_tables", [](MCL &m, const std::vector<uint16_t> &pen, int err_shift, const std::vector<uint32_t> &wtab, int w_shift) {
               MCL::Tables t;
               t.pen = pen;
               t.err_shift = err_shift;
               t.wtab = wtab;
               t.w_shift = w_shift;
               m.setTables(t);
             }, py::arg("pen"), py::arg("err_shift"), py::arg("wtab"), py::arg("w_shift"))
        .def("set_field_model", [](MCL &m, double sigma_hit, int reach, double floor, double pen_scale, int w_shift, int n_w,
                                   uint32_t wtab0, double temperature) {
               MCL::FieldModel d;
               d.sigma_hit = sigma_hit;
               d.reach = reach;
               d.floor = floor;
               d.pen_scale = pen_scale;
               d.w_shift = w_shift;
               d.n_w = n_w;
               d.wtab0 = wtab0;
               d.temperature = temperature;
               m.setFieldModel(d);
             }, py::arg("sigma_hit") = 0.1, py::arg("reach") = 0, py::arg("floor") = 0.05, py::arg("pen_scale") = 64.0,
             py::arg("w_shift") = 4, py::arg("n_w") = 1024, py::arg("wtab0") = 1u << 16, py::arg("temperature") = 256.0,
             "The likelihood-field model (rules 44 and 45) and its tables (judgement); enables the map's distance plane if needed")
        .def("set_field_tables", [](MCL &m, const std::vector<uint16_t> &pen_d2, uint16_t pen_far, int reach,
                                    const std::vector<uint32_t> &wtab, int w_shift) {
               MCL::FieldTables t;
               t.pen_d2 = pen_d2;
               t.pen_far = pen_far;
               t.reach = reach;
               t.wtab = wtab;
               t.w_shift = w_shift;
               m.setFieldTables(t);
             }, py::arg("pen_d2"), py::arg("pen_far"), py::arg("reach"), py::arg("wtab"), py::arg("w_shift"))
        .def_property_readonly("field_model", &MCL::fieldModel)
        .def_static("field_tables", [](float resolution, double sigma_hit, int reach, double floor, double pen_scale, int w_shift,
                                       int n_w, uint32_t wtab0, double temperature) {
               MCL::FieldModel d;
               d.sigma_hit = sigma_hit;
               d.reach = reach;
               d.floor = floor;
               d.pen_scale = pen_scale;
               d.w_shift = w_shift;
               d.n_w = n_w;
               d.wtab0 = wtab0;
               d.temperature = temperature;
               const MCL::FieldTables t = MCL::fieldTables(resolution, d);
               return py::make_tuple(t.pen_d2, t.pen_far, t.reach, t.wtab, t.w_shift);
             }, py::arg("resolution"), py::arg("sigma_hit") = 0.1, py::arg("reach") = 0, py::arg("floor") = 0.05,
             py::arg("pen_scale") = 64.0, py::arg("w_shift") = 4, py::arg("n_w") = 1024, py::arg("wtab0") = 1u << 16,
             py::arg("temperature") = 256.0, "(pen_d2, pen_far, reach, wtab, w_shift) of a field model; needs no device")
        .def("set_motion_noise", &MCL::setMotionNoise, py::arg("sigma_forward"), py::arg("sigma_lateral"), py::arg("sigma_yaw"))
        .def("set_resample_ratio", &MCL::setResampleRatio, py::arg("num"), py::arg("den"))
        .def("set_flags", &MCL::setFlags, py::arg("unknown_blocks") = false, py::arg("skip_no_return") = false)
        .def("set_spread", &MCL::setSpread, py::arg("on"))
        .def("set_recovery", [](MCL &m, int a_slow, int a_fast, uint32_t max_num, uint32_t max_den) {
               MCL::Recovery r;
               r.a_slow = a_slow;
               r.a_fast = a_fast;
               r.max_num = max_num;
               r.max_den = max_den;
               m.setRecovery(r);
             }, py::arg("a_slow") = 4, py::arg("a_fast") = 1, py::arg("max_num") = 1u, py::arg("max_den") = 4u,
             "Recovery by injected free-cell particles (rules 61 to 63); the defaults are judgement, not measurement")
        .def("clear_recovery", &MCL::clearRecovery)
        .def_property_readonly("recovery", &MCL::recovery)
        .def("init", &MCL::init, py::arg("x"), py::arg("y"), py::arg("yaw"), py::arg("sigma_xy"), py::arg("sigma_yaw"))
        .def("init_global", &MCL::initGlobal, "Seed the particles uniformly over the map's empty cells -> their count")
        .def("step", [](MCL &m, const std::array<double, 3> &from, const std::array<double, 3> &to, const std::vector<double> &ranges) {
               py::gil_scoped_release nogil;
               return m.step(from, to, ranges);
             }, py::arg("odom_from"), py::arg("odom_to"), py::arg("ranges"))
        .def("step_quantised", [](MCL &m, int64_t d_f, int64_t d_l, int32_t d_h, int32_t s_f, int32_t s_l, int32_t s_h,
                                  const std::vector<int32_t> &zq, unsigned flags, bool resample) {
               py::gil_scoped_release nogil;
               return m.stepQuantised(d_f, d_l, d_h, s_f, s_l, s_h, zq, flags, resample);
             }, py::arg("d_f"), py::arg("d_l"), py::arg("d_h"), py::arg("s_f"), py::arg("s_l"), py::arg("s_h"), py::arg("zq"),
             py::arg("flags") = 0u, py::arg("resample") = true)
        .def("resample", &MCL::resample)
        .def("particles", [](const MCL &m) {
               const MCL::Particles p = m.particles();
               const py::ssize_t n = static_cast<py::ssize_t>(p.tx.size());
               return py::make_tuple(py::array_t<int64_t>(n, p.tx.data()), py::array_t<int64_t>(n, p.ty.data()),
                                     py::array_t<uint32_t>(n, p.h.data()), py::array_t<uint32_t>(n, p.acc.data()));
             }, "(tx int64, ty int64, h uint32, acc uint32), N each: the states in 2^-16 cells and 2^-16 turns")
        .def_property_readonly("size", &MCL::size)
        .def_property_readonly("beams", &MCL::beams)
        .def_property_readonly("zmax", &MCL::zmax)
        .def_static("noise_scale", &MCL::noiseScale, py::arg("sigma_units"))
        .def_static("quantise_heading", &MCL::quantiseHeading, py::arg("yaw"))
        .def_static("quantise_ranges", &MCL::quantiseRanges, py::arg("ranges"), py::arg("resolution"), py::arg("range_max"),
                    py::arg("flags") = 0u)
        .def_static("odometry_increment", [](float resolution, const std::array<double, 3> &from, const std::array<double, 3> &to) {
               const auto d = MCL::odometryIncrement(resolution, from, to);
               return py::make_tuple(d[0], d[1], d[2]);
             }, py::arg("resolution"), py::arg("odom_from"), py::arg("odom_to"))
        .def_static("estimate_of", [](uint64_t w1, uint64_t w2, uint64_t sx_lo, int64_t sx_hi, uint64_t sy_lo, int64_t sy_hi, int64_t sc,
                                      int64_t ss, int64_t best_tx, int64_t best_ty, float resolution, double origin_x, double origin_y) {
               kc_mcl_record r{};
               r.w1 = w1;
               r.w2 = w2;
               r.sx_lo = sx_lo;
               r.sx_hi = sx_hi;
               r.sy_lo = sy_lo;
               r.sy_hi = sy_hi;
               r.sc = sc;
               r.ss = ss;
               r.best_tx = best_tx;
               r.best_ty = best_ty;
               return MCL::estimateOf(r, resolution, origin_x, origin_y);
             }, "Rule 39 from a record's sums, SX and SY as (lo uint64, hi int64); needs no device")
        .def_static("should_resample", [](uint64_t w1, uint64_t w2, size_t n, uint32_t num, uint32_t den) {
               kc_mcl_record r{};
               r.w1 = w1;
               r.w2 = w2;
               return MCL::shouldResample(r, n, num, den);
             }, py::arg("w1"), py::arg("w2"), py::arg("n"), py::arg("num") = 1u, py::arg("den") = 2u,
             "Rule 40's decision in exact integers; needs no device")
        .def_static("sensor_tables", [](float resolution, double sigma_hit) {
               MCL::Model d;
               d.sigma_hit = sigma_hit;
               const MCL::Tables t = MCL::sensorTables(resolution, d);
               return py::make_tuple(t.pen, t.err_shift, t.wtab, t.w_shift);
             }, py::arg("resolution"), py::arg("sigma_hit") = 0.1, "(pen, err_shift, wtab, w_shift) of the default model");
  }

  // ----------------------------------------------------------------- utils
  // (bindings_utils.cpp:47-129, bindings_gpu.cpp:40-68)
  auto ut = m.def_submodule("utils", "KOMPASS CPP utilities");
  {
    auto czInit = [](auto *tag, CriticalZoneChecker::InputType it, CollisionChecker::ShapeType shape,
                     const std::vector<float> &dims, const py::object &spos, const py::object &srot, float ca,
                     float cd, float sd, const std::vector<double> &angles, float minh, float maxh, float rmax) {
      using T = std::remove_pointer_t<decltype(tag)>;
      return std::make_unique<T>(it, shape, dims, vec3(spos), vec4(srot), ca, cd, sd, angles, minh, maxh, rmax);
    };
    auto worldMapOf = [](const py::object &o) -> const Mapping::WorldMap & {
      const py::object inner = py::hasattr(o, "_map") ? py::object(o.attr("_map")) : o;
      if (!py::isinstance<Mapping::WorldMap>(inner)) throw py::type_error("expected a WorldMap");
      return inner.cast<const Mapping::WorldMap &>();
    };
    py::class_<CriticalZoneChecker> cz(ut, "CriticalZoneChecker");
    py::enum_<CriticalZoneChecker::InputType>(cz, "InputType")
        .value("LASERSCAN", CriticalZoneChecker::InputType::LASERSCAN)
        .value("POINTCLOUD", CriticalZoneChecker::InputType::POINTCLOUD);
    py::enum_<PointFieldType>(ut, "PointFieldType")
        .value("INT8", PointFieldType::INT8).value("UINT8", PointFieldType::UINT8)
        .value("INT16", PointFieldType::INT16).value("UINT16", PointFieldType::UINT16)
        .value("INT32", PointFieldType::INT32).value("UINT32", PointFieldType::UINT32)
        .value("FLOAT32", PointFieldType::FLOAT32).value("FLOAT64", PointFieldType::FLOAT64);
    cz.def(py::init([czInit](CriticalZoneChecker::InputType it, CollisionChecker::ShapeType shape,
                             const std::vector<float> &dims, const py::object &spos, const py::object &srot,
                             float ca, float cd, float sd, const std::vector<double> &angles, float minh,
                             float maxh, float rmax) {
             return czInit(static_cast<CriticalZoneChecker *>(nullptr), it, shape, dims, spos, srot, ca, cd, sd,
                           angles, minh, maxh, rmax);
           }), py::arg("input_type"), py::arg("robot_shape"), py::arg("robot_dimensions"),
           py::arg("sensor_position_body"), py::arg("sensor_rotation_body"), py::arg("critical_angle"),
           py::arg("critical_distance"), py::arg("slowdown_distance"), py::arg("scan_angles"),
           py::arg("min_height"), py::arg("max_height"), py::arg("range_max"))
        .def("check", py::overload_cast<const std::vector<double> &, bool>(&CriticalZoneChecker::check),
             py::arg("ranges"), py::arg("forward"))
        .def("check", py::overload_cast<const std::vector<int8_t> &, int, int, int, int, int, int, int, bool>(
                          &CriticalZoneChecker::check),
             py::arg("data"), py::arg("point_step"), py::arg("row_step"), py::arg("height"), py::arg("width"),
             py::arg("x_offset"), py::arg("y_offset"), py::arg("z_offset"), py::arg("forward"))
        // (not in the reference: the check on a WorldMap's virtual scan at the robot's pose, the ranges on the device)
        // world_map: the class, or the front end's WorldMap that holds one as `_map`
        .def("check", [worldMapOf](CriticalZoneChecker &c, const py::object &world_map, double x, double y, double yaw, bool forward) {
               const Mapping::WorldMap &map = worldMapOf(world_map);
               py::gil_scoped_release nogil;
               return c.check(map, x, y, yaw, forward);
             }, py::arg("world_map"), py::arg("x"), py::arg("y"), py::arg("yaw"), py::arg("forward"))
        .def("check", [worldMapOf](CriticalZoneChecker &c, const py::object &world_map, double x, double y, double yaw, bool forward,
                                   const std::vector<double> &ranges) {
               const Mapping::WorldMap &map = worldMapOf(world_map);
               py::gil_scoped_release nogil;
               return c.check(map, x, y, yaw, forward, ranges);
             }, py::arg("world_map"), py::arg("x"), py::arg("y"), py::arg("yaw"), py::arg("forward"), py::arg("ranges"));
    py::class_<CriticalZoneCheckerGPU, CriticalZoneChecker>(ut, "CriticalZoneCheckerGPU")
        .def(py::init([](CriticalZoneChecker::InputType it, CollisionChecker::ShapeType shape,
                         const std::vector<float> &dims, const py::object &spos, const py::object &srot, float ca,
                         float cd, float sd, const std::vector<double> &angles, float minh, float maxh, float rmax,
                         PointFieldType ft) {
               return std::make_unique<CriticalZoneCheckerGPU>(it, shape, dims, vec3(spos), vec4(srot), ca, cd, sd,
                                                               angles, minh, maxh, rmax, ft);
             }), py::arg("input_type"), py::arg("robot_shape"), py::arg("robot_dimensions"),
             py::arg("sensor_position_body"), py::arg("sensor_rotation_body"), py::arg("critical_angle"),
             py::arg("critical_distance"), py::arg("slowdown_distance"), py::arg("scan_angles"),
             py::arg("min_height"), py::arg("max_height"), py::arg("range_max"),
             py::arg("cloud_field_type") = PointFieldType::FLOAT32);
  }
  ut.def("pointcloud_to_laserscan_from_raw",
         [](const std::vector<int8_t> &data, int point_step, int row_step, int height, int width, int x_offset,
            int y_offset, int z_offset, double max_range, double min_z, double max_z, double angle_step) {
           std::vector<double> ranges_out, angles_out;
           pointCloudToLaserScanFromRaw(data, point_step, row_step, height, width, x_offset, y_offset, z_offset,
                                        max_range, min_z, max_z, angle_step, ranges_out, angles_out);
           return std::make_tuple(ranges_out, angles_out);
         },
         py::arg("data"), py::arg("point_step"), py::arg("row_step"), py::arg("height"), py::arg("width"),
         py::arg("x_offset"), py::arg("y_offset"), py::arg("z_offset"), py::arg("max_range"), py::arg("min_z"),
         py::arg("max_z"), py::arg("angle_step"),
         "Converts raw PointCloud2 to ranges and angles using a specific angular step.");
  ut.def("pointcloud_to_laserscan_from_raw",
         [](const std::vector<int8_t> &data, int point_step, int row_step, int height, int width, int x_offset,
            int y_offset, int z_offset, double max_range, double min_z, double max_z, int num_bins) {
           std::vector<double> ranges_out;
           pointCloudToLaserScanFromRaw(data, point_step, row_step, height, width, x_offset, y_offset, z_offset,
                                        max_range, min_z, max_z, num_bins, ranges_out);
           return ranges_out;
         },
         py::arg("data"), py::arg("point_step"), py::arg("row_step"), py::arg("height"), py::arg("width"),
         py::arg("x_offset"), py::arg("y_offset"), py::arg("z_offset"), py::arg("max_range"), py::arg("min_z"),
         py::arg("max_z"), py::arg("num_bins"),
         "Converts raw PointCloud2 to ranges only, using a fixed number of bins.");
  // read_pcd / read_pcd_to_occupancy_grid (bindings_utils.cpp:122-129)
  ut.def("read_pcd", [](const std::string &filename) {
           std::optional<std::vector<std::array<float, 3>>> pts;
           {
             py::gil_scoped_release nogil;
             pts = readPCD(filename);
           }
           if (!pts) throw std::runtime_error("Failed to read PCD file: " + filename);
           auto *v = new std::vector<std::array<float, 3>>(std::move(*pts));
           py::capsule owner(v, [](void *p) { delete static_cast<std::vector<std::array<float, 3>> *>(p); });
           return py::array_t<float>({(py::ssize_t)v->size(), (py::ssize_t)3}, {(py::ssize_t)12, (py::ssize_t)4},
                                     reinterpret_cast<const float *>(v->data()), owner);
         }, py::arg("filename"), "Convert PCD file to a numpy array of points (zero-copy return).");
  ut.def("read_pcd_to_occupancy_grid", [](const std::string &filename, float grid_resolution, float z_ground_limit,
                                          float robot_height) {
           checkResolution(grid_resolution);
           std::pair<OccupancyGridI8, std::array<float, 3>> r;
           {
             py::gil_scoped_release nogil;
             r = readPCDToOccupancyGrid(filename, grid_resolution, z_ground_limit, robot_height);
           }
           return gridResult(std::move(r));
         }, py::arg("filename"), py::arg("grid_resolution"), py::arg("z_ground_limit"), py::arg("robot_height"),
         "Convert PCD file to an occupancy grid (zero-copy return).");
  // not in the reference: the same grid from a cloud that is already in memory, on the host or on the device
  ut.def("points_to_occupancy_grid", &pointsToGrid, py::arg("points"), py::arg("grid_resolution"),
         py::arg("z_ground_limit"), py::arg("robot_height"),
         "Convert an (N, 3) float32 cloud (numpy array, or a device array read in place) to an occupancy grid.");


  // -------------------------------------------------------------- planning
  // not the reference's OMPL wrapper (planning/ompl.h; out of scope): a deterministic grid planner with that
  // surface's method names where the meaning is the same
  auto pl = m.def_submodule("planning", "Grid planning module");
  py::class_<Planning::GridPlanner>(pl, "GridPlanner")
      .def(py::init([](CollisionChecker::ShapeType shape, const std::vector<float> &dims, bool allow_unknown, float margin) {
             return std::make_unique<Planning::GridPlanner>(shape, dims, allow_unknown, margin);
           }), py::arg("robot_shape"), py::arg("robot_dimensions"), py::arg("allow_unknown") = true,
           py::arg("margin") = 0.0f)
      .def("set_space_bounds_from_map", &Planning::GridPlanner::setSpaceBoundsFromMap, py::arg("origin_x"),
           py::arg("origin_y"), py::arg("width"), py::arg("height"), py::arg("resolution"))
      .def("set_grid", &plannerSetGrid, py::arg("grid"),
           "The (width, height) int32 / int8 grid of the map set before: a numpy array, or a device array read in place")
      .def("set_grid_device", [](Planning::GridPlanner &p, uint64_t ptr, int elem_bytes) {
             py::gil_scoped_release nogil;
             p.setGridOnDevice(reinterpret_cast<const void *>(static_cast<uintptr_t>(ptr)), elem_bytes);
           }, py::arg("device_ptr"), py::arg("elem_bytes") = 4, "A finished grid at a device address, read in place")
      .def("set_grid_from_mapper", &Planning::GridPlanner::setGridFromMapper, py::arg("mapper"),
           "The last grid of a LocalMapper where it lies on the device; takes the bounds from the mapper")
      .def("setup_problem", &Planning::GridPlanner::setupProblem, py::arg("start_x"), py::arg("start_y"),
           py::arg("start_yaw"), py::arg("goal_x"), py::arg("goal_y"), py::arg("goal_yaw"))
      .def("solve", [](Planning::GridPlanner &p, double) {
             py::gil_scoped_release nogil;
             return p.solve();
           }, py::arg("planning_timeout") = 0.0, "planning_timeout is accepted and unused: the solve is exact and bounded")
      .def("replan", [](Planning::GridPlanner &p) {
             py::gil_scoped_release nogil;
             return p.replan();
           }, "solve() from the kept cost field after set_grid* and / or setup_problem with the same goal: the same "
              "outputs, the passes only over what changed; a full solve when nothing can be kept")
      .def("set_grid_from_world_map", [](Planning::GridPlanner &p, const Mapping::WorldMap &map) {
             py::gil_scoped_release nogil;
             return p.setGridFromWorldMap(map);
           }, py::arg("world_map"),
           "The class plane of a WorldMap in place, its metadata read again (DESIGN.md 4.11 rule 51): when its window has been "
           "shifted the bounds and the problem's cells are set again.  -> whether the bounds moved")
      .def("replan", [](Planning::GridPlanner &p, const Mapping::WorldMap &map) {
             py::gil_scoped_release nogil;
             return p.replan(map);
           }, py::arg("world_map"), "set_grid_from_world_map, then replan() -- a full solve() when the bounds moved")
      .def("replanned", &Planning::GridPlanner::replanned, "the last replan() kept a field (false after a full solve)")
      .def("get_replan_threshold", &Planning::GridPlanner::replanThreshold,
           "the last replan()'s rollback threshold in field units; 0xFFFFFFFF when nothing was rolled back")
      .def("get_solution", [](Planning::GridPlanner &p, bool simplify) -> py::object {
             auto path = p.getPath(simplify);
             if (!path) return py::none();
             return py::cast(std::move(*path));
           }, py::arg("simplify") = false)
      .def("get_path_cells", [](Planning::GridPlanner &p, bool simplify) {
             const std::vector<int32_t> ij = p.getPathCells(simplify);
             py::array_t<int32_t> a({(py::ssize_t)(ij.size() / 2), (py::ssize_t)2});
             if (!ij.empty()) std::memcpy(a.mutable_data(), ij.data(), ij.size() * sizeof(int32_t));
             return a;
           }, py::arg("simplify") = false)
      .def("get_cost", &Planning::GridPlanner::getCost)
      .def("get_field", [](Planning::GridPlanner &p) {
             const py::ssize_t w = p.width(), h = p.height();
             py::array_t<uint32_t, py::array::f_style> f({w, h});
             py::array_t<uint8_t, py::array::f_style> v({w, h});
             p.getField(f.mutable_data(), v.mutable_data(), static_cast<size_t>(w) * static_cast<size_t>(h));
             return py::make_tuple(f, v);
           }, "(cost field uint32, validity uint8) of the last solve, [i, j] as the grid")
      .def("set_clearance_cost", &Planning::GridPlanner::setClearanceCost, py::arg("reach"), py::arg("weight"),
           "Surcharge cells within `reach` metres beyond the footprint: `weight` straight-cell lengths at its edge, "
           "falling to 0 at the reach; reach <= 0 or weight <= 0 switches it off")
      .def_static("clearance_table", &Planning::GridPlanner::clearanceTable, py::arg("weight10"), py::arg("r2"), py::arg("c2"),
                  "pen_by_d2[0 .. c2] of set_clearance_cost's rule, in integers")
      .def("get_clearance", [](Planning::GridPlanner &p) {
             const py::ssize_t w = p.width(), h = p.height();
             py::array_t<uint16_t, py::array::f_style> c({w, h});
             py::array_t<uint32_t, py::array::f_style> pen({w, h});
             p.getClearance(c.mutable_data(), pen.mutable_data(), static_cast<size_t>(w) * static_cast<size_t>(h));
             return py::make_tuple(c, pen);
           }, "(clear2 uint16, penalty uint32) of the last solve, [i, j] as the grid; raises with the clearance cost off")
      .def("get_path_min_clearance", &Planning::GridPlanner::getPathMinClearance,
           "metres from the path's cells to the nearest blocking cell; inf when none is within reach")
      .def("get_path_length", &Planning::GridPlanner::getPathLength, "the steps of the path alone, in metres")
      .def("get_any_angle_solution", [](Planning::GridPlanner &p, int max_span) -> py::object {
             auto path = p.getAnyAnglePath(max_span);
             if (!path) return py::none();
             return py::cast(std::move(*path));
           }, py::arg("max_span") = 128,
           "The any-angle path: from each kept cell the farthest of the next max_span cells of the walk in line of sight")
      .def("get_any_angle_cells", [](Planning::GridPlanner &p, int max_span, bool with_indices) -> py::object {
             std::vector<int32_t> idx;
             const std::vector<int32_t> ij = p.getAnyAngleCells(max_span, with_indices ? &idx : nullptr);
             py::array_t<int32_t> a({(py::ssize_t)(ij.size() / 2), (py::ssize_t)2});
             if (!ij.empty()) std::memcpy(a.mutable_data(), ij.data(), ij.size() * sizeof(int32_t));
             if (!with_indices) return a;
             py::array_t<int32_t> b((py::ssize_t)idx.size());
             if (!idx.empty()) std::memcpy(b.mutable_data(), idx.data(), idx.size() * sizeof(int32_t));
             return py::make_tuple(a, b);
           }, py::arg("max_span") = 128, py::arg("with_indices") = false,
           "(k, 2) cells of the any-angle path; with_indices: also their indices into get_path_cells()")
      .def("get_any_angle_length", &Planning::GridPlanner::getAnyAngleLength, py::arg("max_span") = 128,
           "metres along the any-angle path")
      .def("get_any_angle_min_clearance", &Planning::GridPlanner::getAnyAngleMinClearance, py::arg("max_span") = 128,
           "metres from the cells the any-angle path touches to the nearest blocking cell; inf without a clearance cost")
      .def("set_oriented_footprint", &Planning::GridPlanner::setOrientedFootprint, py::arg("on"), py::arg("turn_cost") = 1.0f,
           "Plan over (cell, heading class) with the box's own footprint (BOX robots): moves along the length axis where "
           "the oriented box fits, turns of 45 degrees at `turn_cost` straight-cell lengths where the turning disc fits")
      .def("oriented_on", &Planning::GridPlanner::orientedOn)
      .def("get_oriented_turn10", &Planning::GridPlanner::orientedTurn10)
      .def("get_oriented_a2_b2", [](const Planning::GridPlanner &p) {
             uint32_t a2 = 0, b2 = 0;
             p.orientedA2B2(&a2, &b2);
             return py::make_tuple(a2, b2);
           }, "(A2, B2) of the bounds set; (0, 0) with the mode off")
      .def("get_path_states", [](Planning::GridPlanner &p) {
             const std::vector<int32_t> ijk = p.getPathStates();
             py::array_t<int32_t> a({(py::ssize_t)(ijk.size() / 3), (py::ssize_t)3});
             if (!ijk.empty()) std::memcpy(a.mutable_data(), ijk.data(), ijk.size() * sizeof(int32_t));
             return a;
           }, "(n, 3) states (i, j, k) of the oriented walk; empty without a path or with the mode off")
      .def("get_oriented_field", [](Planning::GridPlanner &p) {
             const py::ssize_t w = p.width(), h = p.height();
             py::array_t<uint32_t> f({(py::ssize_t)4, h, w});  // layer k, then cell (i, j) at i + j * width
             py::array_t<uint8_t, py::array::f_style> v({w, h}), t({w, h});
             p.getOrientedField(f.mutable_data(), v.mutable_data(), t.mutable_data(), static_cast<size_t>(w) * static_cast<size_t>(h));
             return py::make_tuple(f.attr("transpose")(0, 2, 1), v, t);
           }, "(field uint32 [4, i, j], validity bits uint8 [i, j] (bit k = class k), turn validity uint8 [i, j]) of the last oriented solve")
      .def_static("orientation_class", &Planning::GridPlanner::orientationClass, py::arg("yaw"),
                  "The heading class 0 .. 3 of a yaw: ((lround(yaw / (pi / 4)) mod 4) + 4) mod 4")
      .def_static("oriented_mask", [](int k, uint32_t a2, uint32_t b2) {
             const std::vector<int32_t> o = Planning::GridPlanner::orientedMask(k, a2, b2);
             py::array_t<int32_t> a({(py::ssize_t)(o.size() / 2), (py::ssize_t)2});
             if (!o.empty()) std::memcpy(a.mutable_data(), o.data(), o.size() * sizeof(int32_t));
             return a;
           }, py::arg("k"), py::arg("a2"), py::arg("b2"), "The (di, dj) offsets of class k's footprint mask, in integers")
      .def("set_car_motion", &Planning::GridPlanner::setCarMotion, py::arg("on"), py::arg("min_turning_radius") = 0.0f,
           py::arg("allow_reverse") = false, py::arg("reverse_weight") = 2, py::arg("honour_goal_yaw") = true,
           "Plan over (cell, one of eight directed headings) with one straight step and 45-degree arcs whose legs follow "
           "from the minimum turning radius; reverse at `reverse_weight` times the forward cost or not at all; no turn in place")
      .def("car_on", &Planning::GridPlanner::carOn)
      .def("get_car_turn_cells", &Planning::GridPlanner::carTurnCells)
      .def("get_car_reverse_weight", &Planning::GridPlanner::carReverseWeight)
      .def("get_path_moves", [](Planning::GridPlanner &p) {
             const std::vector<int32_t> m = p.getPathMoves();
             py::array_t<int32_t> a({(py::ssize_t)m.size()});
             if (!m.empty()) std::memcpy(a.mutable_data(), m.data(), m.size() * sizeof(int32_t));
             return a;
           }, "(n - 1,) primitive ids (0 .. 5: S, L, R, B, BL, BR) between the states of get_path_states(); empty without a path or with car motion off")
      .def("get_car_field", [](Planning::GridPlanner &p) {
             const py::ssize_t w = p.width(), h = p.height();
             py::array_t<uint32_t> f({(py::ssize_t)8, h, w});  // layer h, then cell (i, j) at i + j * width
             py::array_t<uint8_t> m({(py::ssize_t)8, h, w});
             py::array_t<uint8_t, py::array::f_style> v({w, h});
             p.getCarField(f.mutable_data(), m.mutable_data(), v.mutable_data(), static_cast<size_t>(w) * static_cast<size_t>(h));
             return py::make_tuple(f.attr("transpose")(0, 2, 1), m.attr("transpose")(0, 2, 1), v);
           }, "(field uint32 [8, i, j], moves uint8 [8, i, j] (bit p = primitive p), validity bits uint8 [i, j] (bit h = heading h)) of the last car solve")
      .def_static("heading_class", &Planning::GridPlanner::headingClass, py::arg("yaw"),
                  "The heading 0 .. 7 of a yaw: ((lround(yaw / (pi / 4)) mod 8) + 8) mod 8")
      .def_static("turn_cells", &Planning::GridPlanner::turnCells, py::arg("radius"), py::arg("resolution"),
                  "The legs of a 45-degree arc in cells: max(1, ceil(radius / resolution * tan(pi / 8)))")
      .def("explore", [](Planning::GridPlanner &p, double robot_x, double robot_y, double min_distance, uint32_t min_size) {
             py::gil_scoped_release nogil;
             return p.explore(robot_x, robot_y, min_distance, min_size);
           }, py::arg("robot_x"), py::arg("robot_y"), py::arg("min_distance") = 0.0, py::arg("min_size") = 8,
           "The frontiers of the known map the robot can reach (rules 21 to 26): true when at least one of min_size cells "
           "or more lies min_distance metres or more along the field; raises with a clearance cost or the oriented footprint on")
      .def("get_frontiers", [](Planning::GridPlanner &p) {
             py::list out;
             for (const auto &f : p.frontiers())
               out.append(py::dict(py::arg("entry") = py::make_tuple(f.entry_x, f.entry_y), py::arg("entry_cell") = py::make_tuple(f.entry_i, f.entry_j),
                                   py::arg("centroid") = py::make_tuple(f.centroid_x, f.centroid_y), py::arg("cost") = f.cost,
                                   py::arg("size") = f.size, py::arg("root") = f.root));
             return out;
           }, "The kept frontiers of the last explore(), nearest first: dicts of entry (x, y), entry_cell (i, j), centroid (x, y), "
              "cost in metres, size in cells and root (the label)")
      .def("get_frontier_solution", [](Planning::GridPlanner &p, size_t k) -> py::object {
             auto path = p.frontierPath(k);
             if (!path) return py::none();
             return py::cast(std::move(*path));
           }, py::arg("k"), "The Path from the robot to the entry cell of kept frontier k")
      .def("get_frontier_path_cells", [](Planning::GridPlanner &p, size_t k) {
             const std::vector<int32_t> ij = p.frontierPathCells(k);
             py::array_t<int32_t> a({(py::ssize_t)(ij.size() / 2), (py::ssize_t)2});
             if (!ij.empty()) std::memcpy(a.mutable_data(), ij.data(), ij.size() * sizeof(int32_t));
             return a;
           }, py::arg("k"))
      .def("get_frontier_labels", [](Planning::GridPlanner &p) {
             const py::ssize_t w = p.width(), h = p.height();
             py::array_t<uint32_t, py::array::f_style> l({w, h});
             p.frontierLabels(l.mutable_data(), static_cast<size_t>(w) * static_cast<size_t>(h));
             return l;
           }, "uint32 [i, j]: the label of every frontier cell of the last explore(), 0xFFFFFFFF elsewhere")
      .def("get_components", &Planning::GridPlanner::components, "the frontiers of the last explore(), kept or not")
      .def("get_label_passes", &Planning::GridPlanner::labelPasses)
      .def_static("min_distance_to_cost", &Planning::GridPlanner::minDistanceToCost, py::arg("min_distance"), py::arg("resolution"),
                  "min_cost of explore(): lround(min_distance / resolution * 10), needs no device")
      .def("get_clearance_c2", &Planning::GridPlanner::clearanceC2)
      .def("get_clearance_weight10", &Planning::GridPlanner::clearanceWeight10)
      .def("get_status", &Planning::GridPlanner::status)
      .def("get_passes", &Planning::GridPlanner::passes)
      .def("get_footprint_r2", &Planning::GridPlanner::footprintR2)
      .def("get_cells", [](const Planning::GridPlanner &p) {
             int s[2], g[2];
             p.cells(s, g);
             return py::make_tuple(py::make_tuple(s[0], s[1]), py::make_tuple(g[0], g[1]));
           }, "(start cell, goal cell) of the last setup_problem");

  // ---------------------------------------------------------------- vision
  // (bindings_vision.cpp): the frame goes to kc_depth_boxes by pointer and strides
  auto vi = m.def_submodule("vision", "Vision and Detection module");
  auto compute = [](DepthDetector &self, const py::array &depth_img, const std::vector<Bbox2D> &boxes,
                    float robot_x, float robot_y, float robot_yaw, float robot_speed) {
    const DepthImageView v = depthView(depth_img);
    {
      py::gil_scoped_release nogil;
      self.updateBoxes(v, boxes, std::optional<Path::State>(Path::State(robot_x, robot_y, robot_yaw, robot_speed)));
    }
    return self.get3dDetections().value_or(std::vector<Bbox3D>{});
  };
  py::class_<DepthDetector>(vi, "DepthDetector")
      .def(py::init([](const py::object &depth_range, const py::object &t, const py::object &rot_xyzw,
                       const py::object &focal, const py::object &principal, float factor) {
             const Eigen::Vector4f q = vec4(rot_xyzw);
             return std::make_unique<DepthDetector>(vec2f(depth_range), vec3(t), Eigen::Quaternionf(q(3), q(0), q(1), q(2)),
                                                    vec2f(focal), vec2f(principal), factor);
           }), py::arg("depth_range"), py::arg("camera_in_body_translation"), py::arg("camera_in_body_rotation"),
           py::arg("focal_length"), py::arg("principal_point"), py::arg("depth_conversion_factor") = 1e-3,
           "Initialize with camera translation and rotation (Vector4f as [x, y, z, w]).")
      .def("compute_3d_detections", compute, py::arg("depth_img"), py::arg("input"), py::arg("robot_x"),
           py::arg("robot_y"), py::arg("robot_yaw"), py::arg("robot_speed"))
      .def("compute_3d_detections",
           [compute](DepthDetector &self, const py::array &depth_img, const PointsOfInterest &poi, float robot_x,
                     float robot_y, float robot_yaw, float robot_speed) {
             return compute(self, depth_img, std::vector<Bbox2D>{Bbox2D(poi)}, robot_x, robot_y, robot_yaw,
                            robot_speed);
           },
           py::arg("depth_img"), py::arg("input"), py::arg("robot_x"), py::arg("robot_y"), py::arg("robot_yaw"),
           py::arg("robot_speed"));

  // ---------------------------------------------------------- module level
  py::enum_<LogLevel>(m, "LogLevel")
      .value("DEBUG", LogLevel::DEBUG)
      .value("INFO", LogLevel::INFO)
      .value("WARNING", LogLevel::WARNING)
      .value("WARN", LogLevel::WARNING)
      .value("ERROR", LogLevel::ERROR)
      .export_values();
  m.def("set_log_level", &setLogLevel, "Set the log level");
  m.def("set_log_file", &setLogFile, "Set the log file");
  m.def("comm_unique_id", []() {
    uint8_t id[KC_COMM_ID_BYTES];
    hip::check(kc_comm_unique_id(id));
    return py::bytes(reinterpret_cast<const char *>(id), KC_COMM_ID_BYTES);
  }, "RCCL unique id for DWA.enable_sharding: create on one rank, send to all");
  m.def("set_host_threads", [](int n) { hip::check(kc_set_host_threads(n)); }, py::arg("n"),
        "Threads of the host pool behind the roll-out's libm trig table (default: from the CPUs the process may use)");
  m.def("get_available_accelerators", []() {
    const int n = kc_device_count();
    return n > 0 ? std::string("HIP: ") + std::to_string(n) + " device(s) (gfx950)" : std::string("");
  }, "Get available accelerators");
}
