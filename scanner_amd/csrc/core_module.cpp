// pybind11 bindings: the Python client talks to the C++ engine through this
// module (parity role: scanner/engine/python.cpp). Job specs travel as
// msgpack bytes (packed with the msgpack wheel on the Python side, decoded
// by csrc/msgpack.h here).
#include <dlfcn.h>

#include <chrono>

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "../kernels/dnn.h"
#include "dag/graph.h"
#include "engine/executor.h"
#include "hip_util.h"
#include "memory.h"
#include "msgpack.h"
#include "ops/source.h"
#include "video/h264.h"
#include "video/ingest.h"
#include "video/mp4.h"
#include "ops/dnn_model.h"
#include "ops/image_decode.h"
#include "ops/jpeg_progressive_common.h"
#include "ops/jpeg_common.h"
#include "ops/jpeg_sync_common.h"
#include "ops/kernel.h"
#include "ops/png_common.h"
#include "ops/python_kernel.h"
#include "video/svc.h"

namespace py = pybind11;
using namespace sca;

namespace sca {
// ops/image_encoder.cpp
std::vector<u8> encode_png(const u8* pix, int h, int w, int c);
}  // namespace sca

namespace {

mp::Value mp_from_pybytes(const py::bytes& b) {
  std::string s = b;
  return mp::decode(reinterpret_cast<const u8*>(s.data()), s.size());
}

JobGraph graph_from_bytes(const py::bytes& b) {
  return JobGraph::from_msgpack(mp_from_pybytes(b));
}

std::vector<JobBinding> jobs_from_bytes(const py::bytes& b) {
  std::vector<JobBinding> jobs;
  mp::Value v = mp_from_pybytes(b);
  for (auto& jv : v.as_array()) {
    jobs.push_back(JobBinding::from_msgpack(jv));
  }
  return jobs;
}

PerfParams perf_from_dict(const py::dict& d) {
  PerfParams pp;
  if (d.contains("io_packet_size"))
    pp.io_packet_size = d["io_packet_size"].cast<i64>();
  if (d.contains("work_packet_size"))
    pp.work_packet_size = d["work_packet_size"].cast<i64>();
  if (d.contains("pipeline_instances"))
    pp.pipeline_instances = d["pipeline_instances"].cast<i32>();
  if (d.contains("load_workers"))
    pp.load_workers = d["load_workers"].cast<i32>();
  if (d.contains("cpu_pool_size"))
    pp.cpu_pool_size = d["cpu_pool_size"].cast<size_t>();
  if (d.contains("gpu_pool_size"))
    pp.gpu_pool_size = d["gpu_pool_size"].cast<size_t>();
  if (d.contains("sparsity_threshold"))
    pp.sparsity_threshold = d["sparsity_threshold"].cast<i32>();
  if (d.contains("profiler_level"))
    pp.profiler_level = d["profiler_level"].cast<i32>();
  if (d.contains("span_cache_size"))
    pp.span_cache_size = d["span_cache_size"].cast<size_t>();
  return pp;
}

py::list profilers_to_py(const std::vector<std::unique_ptr<Profiler>>& profs) {
  py::list out;
  for (auto& p : profs) {
    py::dict d;
    py::list iv;
    for (auto& i : p->intervals()) {
      iv.append(py::make_tuple(i.label, i.start_ns, i.end_ns));
    }
    d["intervals"] = iv;
    py::dict cnt;
    for (auto& kv : p->counters()) cnt[py::str(kv.first)] = kv.second;
    d["counters"] = cnt;
    out.append(d);
  }
  return out;
}

// ---- helpers for the kernel test entry points ----

using FArr = py::array_t<float, py::array::c_style | py::array::forcecast>;
const DeviceHandle kTestDev{DeviceType::GPU, 0};

// Device buffer that frees itself (also when a check throws mid-binding).
struct DevBuf {
  u8* p = nullptr;
  size_t bytes = 0;
  explicit DevBuf(size_t n) : bytes(n) {
    if (n) p = new_buffer(kTestDev, n);
  }
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
    return *this;
  }
  ~DevBuf() {
    if (p) delete_buffer(kTestDev, p);
  }
  void poison(void* stream) {
    if (!p) return;
    hipError_t e = hipMemsetAsync(p, 0xFF, bytes, (hipStream_t)stream);
    SCA_CHECK(e == hipSuccess, "test buffer memset failed");
  }
};

std::vector<u16> host_to_bf16(const float* p, size_t n) {
  std::vector<u16> v(n);
  for (size_t i = 0; i < n; ++i) {
    u32 bits;
    std::memcpy(&bits, &p[i], 4);
    bits += 0x7fff + ((bits >> 16) & 1);  // round to nearest even
    v[i] = (u16)(bits >> 16);
  }
  return v;
}

DevBuf upload_bf16(const float* p, size_t n) {
  auto h = host_to_bf16(p, n);
  DevBuf d(n * 2);
  if (n) memcpy_buffer(d.p, kTestDev, (u8*)h.data(), CPU_DEVICE, n * 2);
  return d;
}

DevBuf upload_f32(const float* p, size_t n) {
  DevBuf d(n * 4);
  if (n) memcpy_buffer(d.p, kTestDev, (const u8*)p, CPU_DEVICE, n * 4);
  return d;
}

void bf16_to_host(const DevBuf& d, float* out) {
  size_t n = d.bytes / 2;
  std::vector<u16> h(n);
  memcpy_buffer((u8*)h.data(), CPU_DEVICE, d.p, kTestDev, n * 2);
  for (size_t i = 0; i < n; ++i) {
    u32 bits = (u32)h[i] << 16;
    std::memcpy(&out[i], &bits, 4);
  }
}

py::array_t<float> download_bf16(const DevBuf& d,
                                 std::vector<py::ssize_t> shape) {
  py::array_t<float> out(shape);
  SCA_CHECK((size_t)out.size() * 2 == d.bytes, "download shape mismatch");
  bf16_to_host(d, out.mutable_data());
  return out;
}

// Optional per-column scale/bias (f32 [N]) and residual ([M][N], rounded
// to bf16) of the fused GEMM epilogue.
struct EpilogueBufs {
  DevBuf scale{0}, bias{0}, residual{0};
  EpilogueBufs(const py::object& sc, const py::object& bi,
               const py::object& res, int M, int N) {
    if (!sc.is_none()) {
      FArr a = sc.cast<FArr>();
      SCA_CHECK(a.size() == N, "scale must be [N]");
      scale = upload_f32(a.data(), N);
    }
    if (!bi.is_none()) {
      FArr a = bi.cast<FArr>();
      SCA_CHECK(a.size() == N, "bias must be [N]");
      bias = upload_f32(a.data(), N);
    }
    if (!res.is_none()) {
      FArr a = res.cast<FArr>();
      SCA_CHECK(a.size() == (py::ssize_t)M * N, "residual must be [M][N]");
      residual = upload_bf16(a.data(), (size_t)M * N);
    }
  }
  void apply(GemmArgs& g) const {
    g.scale = (const float*)scale.p;
    g.bias = (const float*)bias.p;
    g.residual = residual.p;
  }
};

// Launch `repeat` times into dC (re-poisoned before each launch) and
// return [M][N], or [repeat][M][N] when repeat > 1.
template <typename F>
py::array_t<float> run_repeated(int repeat, DevBuf& dC, int M, int N,
                                F&& launch) {
  std::vector<py::ssize_t> shape;
  if (repeat > 1) shape.push_back(repeat);
  shape.push_back(M);
  shape.push_back(N);
  py::array_t<float> out(shape);
  void* st = per_thread_hip_stream();
  for (int i = 0; i < repeat; ++i) {
    dC.poison(st);
    launch(st);
    sync_per_thread_stream();
    bf16_to_host(dC, out.mutable_data() + (size_t)i * M * N);
  }
  return out;
}

}  // namespace

PYBIND11_MODULE(_core, m) {
  m.doc() = "scanner_amd C++/HIP engine";

  register_stdlib_ops();
  register_gpu_ops();
  register_resnet50_op();
  register_optflow_gpu();
  register_pose_op();
  register_color_gpu();
  register_image_encoder_op();
  register_image_encoder_gpu();
  register_image_decoder_op();
  register_image_decoder_gpu();
  register_detector_op();
  register_files_source_sink();

  // Load a user op plugin .so built with tools/build_op.py (parity:
  // Client.load_op / REGISTER_OP static registrars in user libraries,
  // scannerpy client.py:514). The dlopen runs the plugin's SCA_REGISTER_*
  // constructors against this module's registries.
  m.def("load_op_library", [](const std::string& path) {
    void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!h) {
      throw ScannerError(std::string("load_op_library failed: ") +
                         dlerror());
    }
  });

  m.def("have_gpu", &have_gpu);
  m.def("gpu_device_count", &gpu_device_count);
  m.def("gpu_free_memory", [](int device) -> size_t {
    SCA_CHECK(have_gpu(), "gpu_free_memory needs a GPU");
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(device);
    size_t free_b = 0, total_b = 0;
    hipError_t e = hipMemGetInfo(&free_b, &total_b);
    (void)hipSetDevice(prev);
    SCA_CHECK(e == hipSuccess, "hipMemGetInfo failed");
    return free_b;
  });

  // GEMM micro-benchmark: device-resident buffers, hipEvent timing.
  // Returns ms per iteration (tools/gemm_tune.py computes TFLOP/s).
  m.def("gemm_bench", [](int M, int N, int K, int iters, bool relu) {
    SCA_CHECK(have_gpu(), "gemm_bench needs a GPU");
    DeviceHandle dev{DeviceType::GPU, 0};
    u8* dA = new_buffer(dev, (size_t)M * K * 2);
    u8* dB = new_buffer(dev, (size_t)N * K * 2);
    u8* dC = new_buffer(dev, (size_t)M * N * 2);
    u8* dS = new_buffer(dev, (size_t)N * 8);
    u8* dSK = new_buffer(dev, 64u << 20);
    splitk_scratch_init(dSK, 64u << 20, nullptr);
    GemmArgs g;
    g.splitk_scratch = dSK;
    g.splitk_scratch_bytes = 64u << 20;
    g.A = dA;
    g.B = dB;
    g.C = dC;
    g.M = M;
    g.N = N;
    g.K = K;
    g.scale = (const float*)dS;
    g.bias = (const float*)(dS + (size_t)N * 4);
    g.relu = relu;
    void* s = per_thread_hip_stream();
    for (int i = 0; i < 3; ++i) gemm_bf16(g, s);
    sync_per_thread_stream();
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, (hipStream_t)s);
    for (int i = 0; i < iters; ++i) gemm_bf16(g, s);
    (void)hipEventRecord(e1, (hipStream_t)s);
    sync_per_thread_stream();
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    delete_buffer(dev, dA);
    delete_buffer(dev, dB);
    delete_buffer(dev, dC);
    delete_buffer(dev, dS);
    delete_buffer(dev, dSK);
    return ms / iters;
  });

  // ---- kernel test entry points (tests/test_dnn_kernels_gpu.py) ----
  // Common shape: host f32 in, rounded to bf16 on the host, run on GPU 0,
  // bf16 out returned as f32. Each call allocates, runs and frees its own
  // buffers; outputs are pre-filled with 0xFF bytes (bf16 NaN) so an
  // element the kernel never wrote cannot pass a comparison.

  // The dispatch plan for a GEMM/conv shape; pure host code, no GPU needed.
  m.def(
      "gemm_plan",
      [](int M, int N, int K, size_t scratch_bytes, bool is_conv) {
        GemmPlan p = gemm_plan(M, N, K, scratch_bytes, is_conv);
        const char* names[] = {"smallk", "splitk", "tile128", "tile64"};
        py::dict d;
        d["kernel"] = names[(int)p.kernel];
        d["splits"] = p.splits;
        d["ksteps_per_split"] = p.ksteps_per_split;
        d["tiles_per_wg"] = p.tiles_per_wg;
        d["grid"] = p.grid;
        d["swizzle"] = p.swizzle;
        d["atomic"] = p.atomic;
        d["fused"] = p.fused;
        return d;
      },
      py::arg("M"), py::arg("N"), py::arg("K"),
      py::arg("scratch_bytes") = 0, py::arg("is_conv") = false);

  // The conv list of "resnet50", "pose1".."pose6" or "detector" as the ops
  // build it,
  // with each conv's place in the device blobs; pure host code, no GPU.
  m.def("dnn_model_specs", [](const std::string& name) {
    std::vector<dnn::ConvSpec> specs;
    if (name == "detector") {
      specs = detector_model_specs();
    } else if (name == "resnet50") {
      specs = resnet50_model_specs();
    } else {
      SCA_CHECK(name.size() == 5 && name.compare(0, 4, "pose") == 0 &&
                    name[4] >= '1' && name[4] <= '6',
                "dnn_model_specs: unknown model '" + name + "'");
      specs = pose_model_specs(name[4] - '0');
    }
    py::list out;
    for (const auto& l : dnn::model_layout(specs)) {
      py::dict d;
      d["name"] = l.spec.name;
      d["in_c"] = l.spec.in_c;
      d["out_c"] = l.spec.out_c;
      d["r"] = l.spec.r;
      d["s"] = l.spec.s;
      d["stride"] = l.spec.stride;
      d["pad"] = l.spec.pad;
      d["relu"] = l.spec.relu;
      d["kp"] = l.spec.kp();
      d["np"] = l.spec.np();
      d["w_off"] = l.w_off;
      d["sb_off"] = l.sb_off;
      out.append(d);
    }
    return out;
  });

  // The Detector op's per-frame host post-process on one frame's f32
  // [1600][64] head maps; returns the BoundingBoxList blob. No GPU.
  m.def(
      "detector_postprocess",
      [](FArr loc, FArr cls, int ih, int iw) {
        SCA_CHECK(loc.ndim() == 2 && loc.shape(0) == 1600 &&
                      loc.shape(1) == 64 && cls.ndim() == 2 &&
                      cls.shape(0) == 1600 && cls.shape(1) == 64,
                  "detector_postprocess: loc and cls must be [1600][64]");
        SCA_CHECK(ih > 0 && iw > 0, "detector_postprocess: bad frame size");
        return py::bytes(detector_postprocess(loc.data(), cls.data(), ih, iw));
      },
      py::arg("loc"), py::arg("cls"), py::arg("ih"), py::arg("iw"));

  // C = act((A @ B_nk^T) * scale + bias + residual). repeat > 1 launches
  // that many times on the same scratch and returns [repeat][M][N].
  m.def(
      "gemm_bf16_test",
      [](FArr A, FArr Bnk, bool relu, py::object scale, py::object bias,
         py::object residual, size_t splitk_scratch_bytes, int repeat) {
        SCA_CHECK(have_gpu(), "gemm_bf16_test needs a GPU");
        SCA_CHECK(A.ndim() == 2 && Bnk.ndim() == 2, "A, B must be 2-D");
        int M = (int)A.shape(0), K = (int)A.shape(1);
        int N = (int)Bnk.shape(0);
        SCA_CHECK((int)Bnk.shape(1) == K, "K mismatch");
        SCA_CHECK(M > 0 && repeat >= 1, "need M > 0 and repeat >= 1");
        DevBuf dA = upload_bf16(A.data(), (size_t)M * K);
        DevBuf dB = upload_bf16(Bnk.data(), (size_t)N * K);
        DevBuf dC((size_t)M * N * 2);
        EpilogueBufs ep(scale, bias, residual, M, N);
        DevBuf dS(splitk_scratch_bytes);
        splitk_scratch_init(dS.p, splitk_scratch_bytes, nullptr);
        GemmArgs g;
        g.A = dA.p;
        g.B = dB.p;
        g.C = dC.p;
        g.M = M;
        g.N = N;
        g.K = K;
        g.relu = relu;
        ep.apply(g);
        g.splitk_scratch = dS.p;
        g.splitk_scratch_bytes = splitk_scratch_bytes;
        return run_repeated(repeat, dC, M, N, [&](void* s) {
          gemm_bf16(g, s);
        });
      },
      py::arg("A"), py::arg("B_nk"), py::arg("relu") = false, py::kw_only(),
      py::arg("scale") = py::none(), py::arg("bias") = py::none(),
      py::arg("residual") = py::none(),
      py::arg("splitk_scratch_bytes") = 0, py::arg("repeat") = 1);

  // Convolution of an NHWC input with weights [N][kp] laid out
  // k = (dr*s+ds)*c + cj, kp = r*s*c padded to x64. implicit=True runs the
  // implicit-GEMM path, implicit=False im2col_bf16 + gemm_bf16. Returns
  // (out [M][N] or [repeat][M][N], im2col matrix [M][kp]); the im2col
  // kernel runs in both modes so its matrix is always returned.
  m.def(
      "conv_bf16_test",
      [](FArr x, FArr w_nk, int r, int s, int stride, int pad,
         py::object scale, py::object bias, py::object residual, bool relu,
         size_t splitk_scratch_bytes, bool implicit, int repeat) {
        SCA_CHECK(have_gpu(), "conv_bf16_test needs a GPU");
        SCA_CHECK(x.ndim() == 4 && w_nk.ndim() == 2, "x NHWC, w [N][kp]");
        SCA_CHECK(r > 0 && s > 0 && stride > 0 && pad >= 0 && repeat >= 1,
                  "bad conv geometry");
        ConvDesc d;
        d.n = (int)x.shape(0);
        d.h = (int)x.shape(1);
        d.w = (int)x.shape(2);
        d.c = (int)x.shape(3);
        d.r = r;
        d.s = s;
        d.stride = stride;
        d.pad = pad;
        SCA_CHECK(d.h + 2 * pad >= r && d.w + 2 * pad >= s,
                  "filter larger than padded input");
        d.oh = (d.h + 2 * pad - r) / stride + 1;
        d.ow = (d.w + 2 * pad - s) / stride + 1;
        int N = (int)w_nk.shape(0), kp = (int)w_nk.shape(1);
        int M = d.n * d.oh * d.ow;
        SCA_CHECK(M > 0 && kp >= r * s * d.c && kp % 64 == 0,
                  "kp must be r*s*c padded to x64");
        DevBuf dX = upload_bf16(x.data(), (size_t)x.size());
        DevBuf dW = upload_bf16(w_nk.data(), (size_t)N * kp);
        DevBuf dC((size_t)M * N * 2);
        DevBuf dCols((size_t)M * kp * 2);
        EpilogueBufs ep(scale, bias, residual, M, N);
        DevBuf dS(splitk_scratch_bytes);
        splitk_scratch_init(dS.p, splitk_scratch_bytes, nullptr);
        void* st = per_thread_hip_stream();
        dCols.poison(st);
        im2col_bf16(dX.p, d.n, d.h, d.w, d.c, r, s, stride, pad, dCols.p,
                    d.oh, d.ow, kp, st);
        GemmArgs g;
        g.A = implicit ? dX.p : dCols.p;
        g.B = dW.p;
        g.C = dC.p;
        g.M = M;
        g.N = N;
        g.K = kp;
        g.relu = relu;
        ep.apply(g);
        g.splitk_scratch = dS.p;
        g.splitk_scratch_bytes = splitk_scratch_bytes;
        py::array_t<float> out = run_repeated(repeat, dC, M, N, [&](void* s2) {
          if (implicit)
            conv_gemm_bf16(g, d, s2);
          else
            gemm_bf16(g, s2);
        });
        return py::make_tuple(out, download_bf16(dCols, {M, kp}));
      },
      py::arg("x_nhwc"), py::arg("w_nk"), py::arg("r"), py::arg("s"),
      py::arg("stride"), py::arg("pad"), py::kw_only(),
      py::arg("scale") = py::none(), py::arg("bias") = py::none(),
      py::arg("residual") = py::none(), py::arg("relu") = false,
      py::arg("splitk_scratch_bytes") = 0, py::arg("implicit") = true,
      py::arg("repeat") = 1);

  m.def("maxpool3x3s2_bf16_test", [](FArr x) {
    SCA_CHECK(have_gpu(), "maxpool3x3s2_bf16_test needs a GPU");
    SCA_CHECK(x.ndim() == 4 && x.size() > 0, "x must be NHWC");
    int n = (int)x.shape(0), h = (int)x.shape(1), w = (int)x.shape(2),
        c = (int)x.shape(3);
    int oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1;
    DevBuf dX = upload_bf16(x.data(), (size_t)x.size());
    DevBuf dO((size_t)n * oh * ow * c * 2);
    void* st = per_thread_hip_stream();
    dO.poison(st);
    maxpool3x3s2_bf16(dX.p, n, h, w, c, dO.p, oh, ow, st);
    sync_per_thread_stream();
    return download_bf16(dO, {n, oh, ow, c});
  });

  m.def("global_avgpool_bf16_test", [](FArr x) {
    SCA_CHECK(have_gpu(), "global_avgpool_bf16_test needs a GPU");
    SCA_CHECK(x.ndim() == 4 && x.size() > 0, "x must be NHWC");
    int n = (int)x.shape(0), h = (int)x.shape(1), w = (int)x.shape(2),
        c = (int)x.shape(3);
    DevBuf dX = upload_bf16(x.data(), (size_t)x.size());
    DevBuf dO((size_t)n * c * 2);
    void* st = per_thread_hip_stream();
    dO.poison(st);
    global_avgpool_bf16(dX.p, n, h, w, c, dO.p, st);
    sync_per_thread_stream();
    return download_bf16(dO, {n, c});
  });

  // x: [n][stride_cols] -> f32 [n][ncols] (exact cast of the bf16 values)
  m.def("bf16_rows_to_f32_test", [](FArr x, int ncols) {
    SCA_CHECK(have_gpu(), "bf16_rows_to_f32_test needs a GPU");
    SCA_CHECK(x.ndim() == 2 && x.size() > 0, "x must be [n][stride_cols]");
    int n = (int)x.shape(0), stride_cols = (int)x.shape(1);
    SCA_CHECK(ncols > 0 && ncols <= stride_cols, "ncols out of range");
    DevBuf dX = upload_bf16(x.data(), (size_t)x.size());
    DevBuf dO((size_t)n * ncols * 4);
    void* st = per_thread_hip_stream();
    dO.poison(st);
    bf16_rows_to_f32(dX.p, n, stride_cols, ncols, dO.p, st);
    sync_per_thread_stream();
    py::array_t<float> out({n, ncols});
    memcpy_buffer((u8*)out.mutable_data(), CPU_DEVICE, dO.p, kTestDev,
                  (size_t)n * ncols * 4);
    return out;
  });

  // a/b/c: [npix][stride] with ca/cb/cc valid channels each
  m.def("concat3_bf16_test", [](FArr a, int ca, FArr b, int cb, FArr c,
                                int cc, int out_stride) {
    SCA_CHECK(have_gpu(), "concat3_bf16_test needs a GPU");
    SCA_CHECK(a.ndim() == 2 && b.ndim() == 2 && c.ndim() == 2,
              "inputs must be [npix][stride]");
    int npix = (int)a.shape(0);
    SCA_CHECK(npix > 0 && b.shape(0) == npix && c.shape(0) == npix,
              "npix mismatch");
    SCA_CHECK(ca >= 0 && cb >= 0 && cc >= 0 && ca <= a.shape(1) &&
                  cb <= b.shape(1) && cc <= c.shape(1) &&
                  out_stride >= ca + cb + cc,
              "channel counts out of range");
    DevBuf dA = upload_bf16(a.data(), (size_t)a.size());
    DevBuf dB = upload_bf16(b.data(), (size_t)b.size());
    DevBuf dCc = upload_bf16(c.data(), (size_t)c.size());
    DevBuf dO((size_t)npix * out_stride * 2);
    void* st = per_thread_hip_stream();
    dO.poison(st);
    concat3_bf16(dA.p, ca, (int)a.shape(1), dB.p, cb, (int)b.shape(1), dCc.p,
                 cc, (int)c.shape(1), npix, dO.p, out_stride, st);
    sync_per_thread_stream();
    return download_bf16(dO, {npix, out_stride});
  });

  // maps: [n][h][w][c_stride] -> f32 [n][nch][3] = {x, y, peak}
  m.def("heatmap_argmax_test", [](FArr maps, int nch) {
    SCA_CHECK(have_gpu(), "heatmap_argmax_test needs a GPU");
    SCA_CHECK(maps.ndim() == 4 && maps.size() > 0, "maps must be NHWC");
    int n = (int)maps.shape(0), h = (int)maps.shape(1),
        w = (int)maps.shape(2), cs = (int)maps.shape(3);
    SCA_CHECK(nch > 0 && nch <= cs, "nch out of range");
    DevBuf dX = upload_bf16(maps.data(), (size_t)maps.size());
    DevBuf dO((size_t)n * nch * 3 * 4);
    void* st = per_thread_hip_stream();
    dO.poison(st);
    heatmap_argmax(dX.p, n, h, w, cs, nch, dO.p, st);
    sync_per_thread_stream();
    py::array_t<float> out({n, nch, 3});
    memcpy_buffer((u8*)out.mutable_data(), CPU_DEVICE, dO.p, kTestDev,
                  (size_t)n * nch * 3 * 4);
    return out;
  });

  // frames: u8 [n][ih][iw][ic]; uploads the frames and the device pointer
  // array itself. Returns [n][out_hw][out_hw][out_c].
  m.def("preprocess_frames_bf16_test",
        [](py::array_t<u8, py::array::c_style | py::array::forcecast> frames,
           int out_hw, int out_c, FArr mean, FArr stdv) {
          SCA_CHECK(have_gpu(), "preprocess_frames_bf16_test needs a GPU");
          SCA_CHECK(frames.ndim() == 4 && frames.size() > 0,
                    "frames must be [n][h][w][c]");
          SCA_CHECK(mean.size() == 3 && stdv.size() == 3 && out_hw > 0 &&
                        out_c >= 3,
                    "need 3 mean/std values and out_c >= 3");
          int n = (int)frames.shape(0), ih = (int)frames.shape(1),
              iw = (int)frames.shape(2), ic = (int)frames.shape(3);
          size_t fbytes = (size_t)ih * iw * ic;
          DevBuf dF(fbytes * n);
          memcpy_buffer(dF.p, kTestDev, frames.data(), CPU_DEVICE,
                        fbytes * n);
          std::vector<const u8*> ptrs(n);
          for (int i = 0; i < n; ++i) ptrs[i] = dF.p + fbytes * i;
          DevBuf dP(sizeof(u8*) * n);
          memcpy_buffer(dP.p, kTestDev, (const u8*)ptrs.data(), CPU_DEVICE,
                        sizeof(u8*) * n);
          float ms[6];
          for (int i = 0; i < 3; ++i) {
            ms[i] = mean.data()[i];
            ms[3 + i] = stdv.data()[i];
          }
          DevBuf dM(sizeof(ms));
          memcpy_buffer(dM.p, kTestDev, (const u8*)ms, CPU_DEVICE,
                        sizeof(ms));
          DevBuf dO((size_t)n * out_hw * out_hw * out_c * 2);
          void* st = per_thread_hip_stream();
          dO.poison(st);
          preprocess_frames_bf16(dP.p, n, ih, iw, ic, out_hw, dO.p,
                                 (const float*)dM.p, (const float*)dM.p + 3,
                                 st, out_c);
          sync_per_thread_stream();
          return download_bf16(dO, {n, out_hw, out_hw, out_c});
        });

  m.def("init_memory", [](size_t cpu_pool, size_t gpu_pool,
                          std::vector<i32> gpu_ids) {
    MemoryConfig cfg;
    cfg.cpu_pool_size = cpu_pool;
    cfg.gpu_pool_size = gpu_pool;
    cfg.gpu_ids = std::move(gpu_ids);
    init_memory_allocators(cfg);
  });
  m.def("destroy_memory", &destroy_memory_allocators);
  // HBM span-cache introspection (tests + profiling)
  m.def("span_cache_stats", [] {
    py::dict d;
    d["hits"] = span_cache_hits();
    d["misses"] = span_cache_misses();
    d["bytes"] = span_cache_bytes_live();
    d["budget"] = span_cache_budget();
    return d;
  });
  // kernel-isolation test: CPU-encode -> GPU-decode -> bytes back (no
  // engine, no cache, no chunking)
  m.def("svc_gpu_debug",
        [](py::array_t<u8, py::array::c_style | py::array::forcecast> frames) {
          i64 n = frames.shape(0);
          i32 h = (i32)frames.shape(1), w = (i32)frames.shape(2),
              c = (i32)frames.shape(3);
          VideoMetadata vm;
          std::vector<u8> stream;
          svc_encode_cpu(frames.data(), n, h, w, c, 16, stream, vm);
          py::dict r;
          r["dev"] = svc_gpu_debug_dump(stream, vm);
          // host-side expectations for supers 255..257, frame 0
          u32 nbytes = (u32)((i64)h) * w * c;
          u32 ngroups = (nbytes + 31) / 32;
          u32 nsuper = (ngroups + 127) / 128;
          const u8* pkt = stream.data() + vm.sample_offsets[0];
          const u32* so = (const u32*)(pkt + 20);
          u64 widths_off = 20ull + (u64)nsuper * 4;
          u64 packed_off = widths_off + (ngroups + 3) / 4 * 4;
          py::list host;
          for (u32 s = 255; s <= 257; ++s) {
            u32 g0 = s * 128;
            u32 wv = pkt[widths_off + g0];
            const u32* q = (const u32*)(pkt + packed_off + so[s]);
            py::dict e;
            e["super_off"] = so[s];
            e["w_lane0"] = wv;
            e["q0"] = q[0];
            e["q1"] = q[1];
            e["packed_off"] = (u32)packed_off;
            host.append(e);
          }
          r["host"] = host;
          return r;
        });
  m.def("svc_gpu_roundtrip",
        [](py::array_t<u8, py::array::c_style | py::array::forcecast> frames,
           i32 gop, std::vector<i64> want) {
          SCA_CHECK(frames.ndim() == 4, "frames must be [N,H,W,C]");
          i64 n = frames.shape(0);
          i32 h = (i32)frames.shape(1), w = (i32)frames.shape(2),
              c = (i32)frames.shape(3);
          VideoMetadata vm;
          std::vector<u8> stream;
          svc_encode_cpu(frames.data(), n, h, w, c, gop, stream, vm);
          if (want.empty())
            for (i64 i = 0; i < n; ++i) want.push_back(i);
          DeviceHandle dev{DeviceType::GPU, 0};
          auto elems = svc_decode_gpu(stream.data(), stream.size(), vm,
                                      want, dev, 0);
          py::array_t<u8> out({(i64)elems.size(), (i64)h, (i64)w, (i64)c});
          size_t fsize = (size_t)h * w * c;
          for (size_t i = 0; i < elems.size(); ++i) {
            memcpy_buffer(out.mutable_data() + i * fsize, CPU_DEVICE,
                          elems[i].buffer, dev, fsize);
            delete_buffer(dev, elems[i].buffer);
          }
          return out;
        },
        py::arg("frames"), py::arg("gop") = 16,
        py::arg("want") = std::vector<i64>{});
  // ---- sink-side SVC encode (kernels/svc_encode.hip) ----
  m.def("svc_packet_bound", &svc_packet_bound, py::arg("nbytes"));
  // the oracle: svc_encode_cpu -> (stream bytes, per-frame packet sizes)
  m.def("svc_cpu_encode",
        [](py::array_t<u8, py::array::c_style | py::array::forcecast> frames,
           i32 gop) {
          SCA_CHECK(frames.ndim() == 4, "frames must be [N,H,W,C]");
          SCA_CHECK(gop >= 1, "gop must be >= 1");
          VideoMetadata vm;
          std::vector<u8> stream;
          svc_encode_cpu(frames.data(), frames.shape(0), (i32)frames.shape(1),
                         (i32)frames.shape(2), (i32)frames.shape(3), gop,
                         stream, vm);
          return py::make_tuple(
              py::bytes((const char*)stream.data(), stream.size()),
              vm.sample_sizes);
        },
        py::arg("frames"), py::arg("gop") = 16);
  // CPU decode of a packet stream given its per-frame sizes (checks the
  // GPU encoder's output with the CPU decoder alone)
  // `keyframes`, when given, is the explicit sorted list of key frame
  // indices and replaces the `gop` period; `want` defaults to every frame.
  m.def("svc_cpu_decode",
        [](py::bytes stream_b, std::vector<u64> sizes, i32 h, i32 w, i32 c,
           i32 gop, std::optional<std::vector<i64>> keyframes,
           std::optional<std::vector<i64>> want_opt) {
          std::string stream = stream_b;
          SCA_CHECK(gop >= 1, "gop must be >= 1");
          VideoMetadata vm;
          vm.codec = "svc";
          vm.height = h;
          vm.width = w;
          vm.channels = c;
          vm.frame_type = FrameType::U8;
          vm.num_frames = (i64)sizes.size();
          u64 off = 0;
          std::vector<i64> want;
          for (size_t i = 0; i < sizes.size(); ++i) {
            if (!keyframes && i % gop == 0)
              vm.keyframe_indices.push_back((i64)i);
            vm.sample_offsets.push_back(off);
            vm.sample_sizes.push_back(sizes[i]);
            off += sizes[i];
            want.push_back((i64)i);
          }
          if (keyframes) vm.keyframe_indices = *keyframes;
          if (want_opt) want = *want_opt;
          SCA_CHECK(off == stream.size(), "sizes do not add up to the stream");
          std::vector<std::vector<u8>> frames;
          svc_decode_cpu((const u8*)stream.data(), stream.size(), vm, want,
                         frames);
          size_t fsize = (size_t)h * w * c;
          py::array_t<u8> out({(i64)frames.size(), (i64)h, (i64)w, (i64)c});
          for (size_t i = 0; i < frames.size(); ++i)
            std::memcpy(out.mutable_data() + i * fsize, frames[i].data(),
                        fsize);
          return out;
        },
        py::arg("stream"), py::arg("sizes"), py::arg("h"), py::arg("w"),
        py::arg("c"), py::arg("gop") = 16, py::arg("keyframes") = py::none(),
        py::arg("want") = py::none());
  // GPU decode of any packet stream, the way the executor calls it.
  // resident=False: the bytes [offset(first), end of the span's last packet)
  // go into a pinned CPU-pool buffer and svc_decode_gpu uploads what it
  // needs (stream_offset = offset(first)). resident=True: the bytes from
  // offset(first) on are uploaded first and svc_decode_gpu_dev decodes from
  // them (dev_lo = offset(first)), the span-cache path. Returns the wanted
  // frames; every buffer it took is back in its pool on return or throw.
  m.def("svc_gpu_decode",
        [](py::bytes stream_b, std::vector<u64> sizes, i32 h, i32 w, i32 c,
           std::vector<i64> keyframes, std::vector<i64> want, bool resident,
           i64 first) {
          std::string stream = stream_b;
          SCA_CHECK(h > 0 && w > 0 && c > 0, "bad frame geometry");
          VideoMetadata vm;
          vm.codec = "svc";
          vm.height = h;
          vm.width = w;
          vm.channels = c;
          vm.frame_type = FrameType::U8;
          vm.num_frames = (i64)sizes.size();
          vm.keyframe_indices = keyframes;
          u64 total = 0;
          for (u64 sz : sizes) {
            vm.sample_offsets.push_back(total);
            vm.sample_sizes.push_back(sz);
            total += sz;
          }
          SCA_CHECK(total == stream.size(),
                    "sizes do not add up to the stream");
          i64 n = (i64)sizes.size();
          if (first < 0) first = 0;
          SCA_CHECK(first == 0 || first < n, "first beyond stream");
          size_t fsize = (size_t)h * w * c;
          py::array_t<u8> out({(i64)want.size(), (i64)h, (i64)w, (i64)c});
          u8* out_p = out.mutable_data();
          {
            py::gil_scoped_release rel;
            DeviceHandle dev{DeviceType::GPU, 0};
            std::vector<i64> span = svc_decode_span(vm, want);
            u64 lo = n > 0 ? vm.sample_offsets[first] : 0;
            // a span frame the stream does not hold is the decoder's to
            // reject; here it only must not index past the tables
            u64 hi = total;
            if (!resident && !span.empty() && span.back() >= 0 &&
                span.back() < n)
              hi = vm.sample_offsets[span.back()] +
                   vm.sample_sizes[span.back()];
            if (hi < lo) hi = lo;
            size_t nb = (size_t)(hi - lo);
            const u8* src = (const u8*)stream.data() + lo;
            u8* h_stream = nullptr;
            u8* d_stream = nullptr;
            std::vector<Element> elems;
            try {
              if (resident) {
                d_stream = new_buffer(dev, nb ? nb : 1);
                if (nb) memcpy_buffer(d_stream, dev, src, CPU_DEVICE, nb);
                elems = svc_decode_gpu_dev(d_stream, lo, vm, want, dev);
              } else {
                h_stream = new_buffer(CPU_DEVICE, nb ? nb : 1);
                std::memcpy(h_stream, src, nb);
                elems = svc_decode_gpu(h_stream, nb, vm, want, dev, lo);
              }
              SCA_CHECK(elems.size() == want.size(),
                        "svc_gpu_decode: frame count mismatch");
              // one copy per frame: the frames are allocations of their
              // own, which memcpy_vec would coalesce when they lie adjacent
              for (size_t i = 0; i < elems.size(); ++i)
                memcpy_buffer(out_p + i * fsize, CPU_DEVICE, elems[i].buffer,
                              dev, fsize);
            } catch (...) {
              for (auto& e : elems) delete_buffer(dev, e.buffer);
              if (d_stream) delete_buffer(dev, d_stream);
              if (h_stream) delete_buffer(CPU_DEVICE, h_stream);
              throw;
            }
            for (auto& e : elems) delete_buffer(dev, e.buffer);
            if (d_stream) delete_buffer(dev, d_stream);
            if (h_stream) delete_buffer(CPU_DEVICE, h_stream);
          }
          return out;
        },
        py::arg("stream"), py::arg("sizes"), py::arg("h"), py::arg("w"),
        py::arg("c"), py::arg("keyframes"), py::arg("want"),
        py::arg("resident") = false, py::arg("first") = 0);
  // The clip is uploaded as ONE contiguous device buffer (frame i at
  // i*nbytes), so an odd nbytes gives misaligned frames. chunk > 0 splits
  // the encode into consecutive calls of `chunk` frames, each predicting its
  // first delta frame from the previous call's last frame — the executor's
  // packet pattern.
  m.def("svc_gpu_encode",
        [](py::array_t<u8, py::array::c_style | py::array::forcecast> frames,
           i32 gop, i64 chunk) {
          SCA_CHECK(frames.ndim() == 4, "frames must be [N,H,W,C]");
          SCA_CHECK(gop >= 1, "gop must be >= 1");
          i64 n = frames.shape(0);
          size_t fsize = (size_t)frames.shape(1) * frames.shape(2) *
                         frames.shape(3);
          DeviceHandle dev{DeviceType::GPU, 0};
          std::vector<u8> stream;
          std::vector<u64> sizes;
          if (n == 0) {
            return py::make_tuple(py::bytes(), sizes);
          }
          u8* d = new_buffer(dev, fsize * n);
          try {
            memcpy_buffer(d, dev, frames.data(), CPU_DEVICE, fsize * n);
            i64 step = chunk > 0 ? chunk : n;
            for (i64 s = 0; s < n; s += step) {
              i64 e = std::min(n, s + step);
              std::vector<const u8*> fp;
              std::vector<u8> key;
              for (i64 i = s; i < e; ++i) {
                fp.push_back(d + (size_t)i * fsize);
                key.push_back(i % gop == 0 ? 1 : 0);
              }
              svc_encode_gpu(fp, s > 0 ? d + (size_t)(s - 1) * fsize : nullptr,
                             key, (u32)fsize, dev, stream, sizes);
            }
          } catch (...) {
            delete_buffer(dev, d);
            throw;
          }
          delete_buffer(dev, d);
          return py::make_tuple(
              py::bytes((const char*)stream.data(), stream.size()), sizes);
        },
        py::arg("frames"), py::arg("gop") = 16, py::arg("chunk") = 0);
  // Seconds for `iters` encodes of n device-resident h*w*c frames, ending in
  // a stream synchronise. mode "gpu": svc_encode_gpu including the D2H of
  // the compressed bytes. mode "cpu": the host sink path — D2H of the raw
  // frames into host memory, then svc_encode_cpu. clip "smooth" is a moving
  // gradient (small widths), "noise" a seeded xorshift stream (width 8).
  m.def("svc_encode_bench",
        [](i32 h, i32 w, i32 c, i64 n, i32 iters, const std::string& mode,
           const std::string& clip, u32 seed) {
          SCA_CHECK(mode == "gpu" || mode == "cpu",
                    "mode must be 'gpu' or 'cpu'");
          SCA_CHECK(clip == "smooth" || clip == "noise",
                    "clip must be 'smooth' or 'noise'");
          size_t fsize = (size_t)h * w * c;
          SCA_CHECK(n > 0 && fsize > 0 && iters > 0, "empty benchmark");
          DeviceHandle dev{DeviceType::GPU, 0};
          // one block buffer, as a kernel op's output batch would be
          u8* d = new_block_buffer(dev, fsize * n, 1);
          double secs = 0;
          try {
            {
              std::vector<u8> host(fsize * n);
              u32 x = seed * 2654435761u + 1u;
              size_t p = 0;
              for (i64 i = 0; i < n; ++i)
                for (i32 y = 0; y < h; ++y)
                  for (i32 xx = 0; xx < w; ++xx)
                    for (i32 ch = 0; ch < c; ++ch, ++p) {
                      if (clip == "noise") {
                        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
                        host[p] = (u8)(x >> 24);
                      } else {
                        i64 v = ch % 3 == 0   ? xx + i * 2
                                : ch % 3 == 1 ? y + i
                                              : xx + y + i * 3;
                        host[p] = (u8)((v + seed) & 0xff);
                      }
                    }
              memcpy_buffer(d, dev, host.data(), CPU_DEVICE, fsize * n);
            }
            std::vector<const u8*> fp;
            std::vector<u8> key;
            for (i64 i = 0; i < n; ++i) {
              fp.push_back(d + (size_t)i * fsize);
              key.push_back(i % 16 == 0 ? 1 : 0);
            }
            py::gil_scoped_release rel;
            auto t0 = std::chrono::steady_clock::now();
            for (i32 it = 0; it < iters; ++it) {
              std::vector<u8> stream;
              if (mode == "gpu") {
                std::vector<u64> sizes;
                svc_encode_gpu(fp, nullptr, key, (u32)fsize, dev, stream,
                               sizes);
              } else {
                // executor sink today: per-frame pinned host elements, one
                // batched D2H, then concatenate + encode
                std::vector<u8*> dst;
                std::vector<size_t> sz;
                for (i64 i = 0; i < n; ++i) {
                  dst.push_back(new_buffer(CPU_DEVICE, fsize));
                  sz.push_back(fsize);
                }
                memcpy_vec(dst, CPU_DEVICE, fp, dev, sz);
                std::vector<u8> contig;
                contig.reserve(fsize * n);
                for (i64 i = 0; i < n; ++i) {
                  contig.insert(contig.end(), dst[i], dst[i] + fsize);
                  delete_buffer(CPU_DEVICE, dst[i]);
                }
                VideoMetadata vm;
                svc_encode_cpu(contig.data(), n, h, w, c, 16, stream, vm);
              }
              sync_per_thread_stream();
            }
            secs = std::chrono::duration<double>(
                       std::chrono::steady_clock::now() - t0)
                       .count();
          } catch (...) {
            delete_buffer(dev, d);
            throw;
          }
          delete_buffer(dev, d);
          return secs;
        },
        py::arg("h"), py::arg("w"), py::arg("c"), py::arg("n"),
        py::arg("iters") = 1, py::arg("mode") = "gpu",
        py::arg("clip") = "smooth", py::arg("seed") = 0);
  // ---- JPEG still-image encode (ops/jpeg_cpu.cpp, kernels/jpeg_encode.hip)
  // every binding below takes subsampling = "444" | "420" last
  m.def("jpeg_restart_interval",
        [](const std::string& subsampling) {
          return jpeg_parse_subsampling(subsampling) == JpegSubsampling::k420
                     ? kJpegRestartInterval420
                     : kJpegRestartInterval;
        },
        py::arg("subsampling") = "444");
  m.def("jpeg_size_bound",
        [](i32 h, i32 w, i32 c, const std::string& subsampling) {
          return jpeg_size_bound(h, w, c, jpeg_parse_subsampling(subsampling));
        },
        py::arg("h"), py::arg("w"), py::arg("c"),
        py::arg("subsampling") = "444");
  // the oracle: one [H,W,C] u8 frame -> file bytes
  m.def("jpeg_cpu_encode",
        [](py::array_t<u8, py::array::c_style | py::array::forcecast> frame,
           i32 quality, const std::string& subsampling) {
          SCA_CHECK(frame.ndim() == 3, "frame must be [H,W,C]");
          auto v = jpeg_encode_cpu(frame.data(), (i32)frame.shape(0),
                                   (i32)frame.shape(1), (i32)frame.shape(2),
                                   quality,
                                   jpeg_parse_subsampling(subsampling));
          return py::bytes((const char*)v.data(), v.size());
        },
        py::arg("frame"), py::arg("quality") = 90,
        py::arg("subsampling") = "444");
  // quantised coefficients, int16 [ncomp, by, bx, 64] in zig-zag order. A
  // 3-channel frame with subsampling="420" gives a tuple of two arrays on
  // their own block grids: Y [2*mcus_y, 2*mcus_x, 64] and chroma
  // [2, mcus_y, mcus_x, 64] (Cb, Cr), mcus_* counting 16x16-pixel MCUs.
  m.def("jpeg_quantize_cpu",
        [](py::array_t<u8, py::array::c_style | py::array::forcecast> frame,
           i32 quality, const std::string& subsampling) -> py::object {
          SCA_CHECK(frame.ndim() == 3, "frame must be [H,W,C]");
          i32 h = (i32)frame.shape(0), w = (i32)frame.shape(1),
              c = (i32)frame.shape(2);
          jpeg_check_args(h, w, c, quality);
          JpegTables t;
          jpeg_make_tables(c, quality, t);
          JpegGeom g =
              jpeg_geom(h, w, c, jpeg_parse_subsampling(subsampling));
          i16 zz[64];
          if (g.ss == JpegSubsampling::k420) {
            py::array_t<i16> ya(
                {(i64)g.mcus_y * 2, (i64)g.mcus_x * 2, (i64)64});
            py::array_t<i16> ca(
                {(i64)2, (i64)g.mcus_y, (i64)g.mcus_x, (i64)64});
            i16* o = ya.mutable_data();
            for (u32 by = 0; by < g.mcus_y * 2; ++by)
              for (u32 bx = 0; bx < g.mcus_x * 2; ++bx, o += 64) {
                jpeg_block_coefs(frame.data(), h, w, c, bx, by, 0, t, zz);
                std::memcpy(o, zz, sizeof(zz));
              }
            o = ca.mutable_data();
            for (i32 comp = 1; comp < 3; ++comp)
              for (u32 by = 0; by < g.mcus_y; ++by)
                for (u32 bx = 0; bx < g.mcus_x; ++bx, o += 64) {
                  jpeg_block_coefs_420(frame.data(), h, w, bx, by, comp, t,
                                       zz);
                  std::memcpy(o, zz, sizeof(zz));
                }
            return py::make_tuple(ya, ca);
          }
          py::array_t<i16> out(
              {(i64)c, (i64)g.mcus_y, (i64)g.mcus_x, (i64)64});
          i16* o = out.mutable_data();
          for (i32 comp = 0; comp < c; ++comp)
            for (u32 by = 0; by < g.mcus_y; ++by)
              for (u32 bx = 0; bx < g.mcus_x; ++bx, o += 64) {
                jpeg_block_coefs(frame.data(), h, w, c, bx, by, comp, t, zz);
                std::memcpy(o, zz, sizeof(zz));
              }
          return out;
        },
        py::arg("frame"), py::arg("quality") = 90,
        py::arg("subsampling") = "444");
  // [N,H,W,C] u8 frames are uploaded as ONE contiguous device buffer (frame
  // i at i*H*W*C, so an odd frame size gives misaligned frames) and encoded
  // in one call -> list of file bytes
  m.def("jpeg_gpu_encode",
        [](py::array_t<u8, py::array::c_style | py::array::forcecast> frames,
           i32 quality, const std::string& subsampling) {
          JpegSubsampling ss = jpeg_parse_subsampling(subsampling);
          SCA_CHECK(have_gpu(), "jpeg_gpu_encode needs a GPU");
          SCA_CHECK(frames.ndim() == 4, "frames must be [N,H,W,C]");
          i64 n = frames.shape(0);
          i32 h = (i32)frames.shape(1), w = (i32)frames.shape(2),
              c = (i32)frames.shape(3);
          jpeg_check_args(h, w, c, quality);
          size_t fsize = (size_t)h * w * c;
          DeviceHandle dev{DeviceType::GPU, 0};
          py::list res;
          if (n == 0) return res;
          u8* d = new_buffer(dev, fsize * n);
          std::vector<u8*> bufs;
          std::vector<u64> sizes;
          try {
            memcpy_buffer(d, dev, frames.data(), CPU_DEVICE, fsize * n);
            std::vector<const u8*> fp;
            for (i64 i = 0; i < n; ++i) fp.push_back(d + (size_t)i * fsize);
            jpeg_encode_gpu(fp, h, w, c, quality, dev, per_thread_hip_stream(),
                            bufs, sizes, ss);
            for (size_t i = 0; i < bufs.size(); ++i) {
              std::string host(sizes[i], '\0');
              memcpy_buffer((u8*)host.data(), CPU_DEVICE, bufs[i], dev,
                            sizes[i]);
              res.append(py::bytes(host));
            }
          } catch (...) {
            for (u8* b : bufs) delete_buffer(dev, b);
            delete_buffer(dev, d);
            throw;
          }
          for (u8* b : bufs) delete_buffer(dev, b);
          delete_buffer(dev, d);
          return res;
        },
        py::arg("frames"), py::arg("quality") = 90,
        py::arg("subsampling") = "444");
  // Seconds for `iters` encodes of `batch` device-resident h*w*c frames,
  // each ending with the files in host memory. mode "gpu": jpeg_encode_gpu,
  // then D2H of the compressed bytes. mode "cpu": D2H of the raw frames,
  // then jpeg_encode_cpu. mode "png": D2H of the raw frames, then the PNG
  // writer (the only image path before the JPEG encoder). Also returns the
  // bytes produced by one iteration. clip: "smooth" gradients or "noise".
  // subsampling applies to the two JPEG modes.
  m.def("jpeg_encode_bench",
        [](i32 h, i32 w, i32 c, i32 quality, i64 batch, i32 iters,
           const std::string& mode, const std::string& clip,
           const std::string& subsampling) {
          JpegSubsampling ss = jpeg_parse_subsampling(subsampling);
          SCA_CHECK(have_gpu(), "jpeg_encode_bench needs a GPU");
          SCA_CHECK(mode == "gpu" || mode == "cpu" || mode == "png",
                    "mode must be 'gpu', 'cpu' or 'png'");
          SCA_CHECK(clip == "smooth" || clip == "noise",
                    "clip must be 'smooth' or 'noise'");
          jpeg_check_args(h, w, c, quality);
          SCA_CHECK(batch > 0 && iters > 0, "empty benchmark");
          size_t fsize = (size_t)h * w * c;
          DeviceHandle dev{DeviceType::GPU, 0};
          u8* d = new_block_buffer(dev, fsize * batch, 1);
          double secs = 0;
          u64 out_bytes = 0;
          try {
            {
              std::vector<u8> host(fsize * batch);
              u32 x = 2654435761u;
              size_t p = 0;
              for (i64 i = 0; i < batch; ++i)
                for (i32 y = 0; y < h; ++y)
                  for (i32 xx = 0; xx < w; ++xx)
                    for (i32 ch = 0; ch < c; ++ch, ++p) {
                      if (clip == "noise") {
                        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
                        host[p] = (u8)(x >> 24);
                      } else {
                        i64 v = ch % 3 == 0   ? xx + i * 2
                                : ch % 3 == 1 ? y + i
                                              : (xx + y) / 2 + i * 3;
                        host[p] = (u8)(v & 0xff);
                      }
                    }
              memcpy_buffer(d, dev, host.data(), CPU_DEVICE, fsize * batch);
            }
            std::vector<const u8*> fp;
            for (i64 i = 0; i < batch; ++i) fp.push_back(d + (size_t)i * fsize);
            py::gil_scoped_release rel;
            auto t0 = std::chrono::steady_clock::now();
            for (i32 it = 0; it < iters; ++it) {
              out_bytes = 0;
              if (mode == "gpu") {
                std::vector<u8*> bufs;
                std::vector<u64> sizes;
                jpeg_encode_gpu(fp, h, w, c, quality, dev,
                                per_thread_hip_stream(), bufs, sizes, ss);
                std::vector<u8*> dst;
                std::vector<const u8*> src(bufs.begin(), bufs.end());
                std::vector<size_t> sz(sizes.begin(), sizes.end());
                for (u64 s : sizes) {
                  dst.push_back(new_buffer(CPU_DEVICE, s));
                  out_bytes += s;
                }
                memcpy_vec(dst, CPU_DEVICE, src, dev, sz);
                for (u8* b : dst) delete_buffer(CPU_DEVICE, b);
                for (u8* b : bufs) delete_buffer(dev, b);
              } else {
                std::vector<u8*> dst;
                std::vector<size_t> sz(batch, fsize);
                for (i64 i = 0; i < batch; ++i)
                  dst.push_back(new_buffer(CPU_DEVICE, fsize));
                memcpy_vec(dst, CPU_DEVICE, fp, dev, sz);
                for (i64 i = 0; i < batch; ++i) {
                  auto v = mode == "cpu"
                               ? jpeg_encode_cpu(dst[i], h, w, c, quality, ss)
                               : encode_png(dst[i], h, w, c);
                  out_bytes += v.size();
                  delete_buffer(CPU_DEVICE, dst[i]);
                }
              }
            }
            secs = std::chrono::duration<double>(
                       std::chrono::steady_clock::now() - t0)
                       .count();
          } catch (...) {
            delete_buffer(dev, d);
            throw;
          }
          delete_buffer(dev, d);
          return py::make_tuple(secs, out_bytes);
        },
        py::arg("h"), py::arg("w"), py::arg("c"), py::arg("quality") = 90,
        py::arg("batch") = 8, py::arg("iters") = 1, py::arg("mode") = "gpu",
        py::arg("clip") = "smooth", py::arg("subsampling") = "444");
  // ---- PNG encode (ops/image_encoder.cpp, ops/png_encode_cpu.cpp,
  // kernels/png_encode.hip)
  m.def("png_chunk_bytes", []() { return kPngChunkBytes; });
  m.def("png_size_bound", [](i32 h, i32 w, i32 c) {
    png_check_args(h, w, c);
    return png_size_bound(h, w, c);
  }, py::arg("h"), py::arg("w"), py::arg("c"));
  // one [H,W,C] u8 frame -> file bytes, writer = "zlib" | "parallel"
  m.def("png_cpu_encode",
        [](py::array_t<u8, py::array::c_style | py::array::forcecast> frame,
           const std::string& writer) {
          SCA_CHECK(frame.ndim() == 3, "frame must be [H,W,C]");
          i32 h = (i32)frame.shape(0), w = (i32)frame.shape(1),
              c = (i32)frame.shape(2);
          auto v = png_parse_writer(writer) == PngWriter::kParallel
                       ? png_encode_parallel_cpu(frame.data(), h, w, c)
                       : encode_png(frame.data(), h, w, c);
          return py::bytes((const char*)v.data(), v.size());
        },
        py::arg("frame"), py::arg("writer") = "zlib");
  // a list of [H,W,C] u8 frames, shapes may differ -> list of file bytes
  // ("parallel" writer). Every frame is uploaded on its own; consecutive
  // frames of one shape are encoded in one call, as the op does.
  m.def("png_gpu_encode", [](py::list frames) {
    SCA_CHECK(have_gpu(), "png_gpu_encode needs a GPU");
    using Arr = py::array_t<u8, py::array::c_style | py::array::forcecast>;
    DeviceHandle dev{DeviceType::GPU, 0};
    std::vector<Arr> arrs;
    for (py::handle f : frames) {
      arrs.push_back(f.cast<Arr>());
      SCA_CHECK(arrs.back().ndim() == 3, "frames must be [H,W,C]");
      png_check_args((i32)arrs.back().shape(0), (i32)arrs.back().shape(1),
                     (i32)arrs.back().shape(2));
    }
    std::vector<u8*> dfr, bufs;
    std::vector<u64> sizes;
    py::list res;
    auto cleanup = [&]() {
      for (u8* b : bufs) delete_buffer(dev, b);
      for (u8* b : dfr) delete_buffer(dev, b);
    };
    try {
      for (const Arr& a : arrs) {
        dfr.push_back(new_buffer(dev, (size_t)a.size()));
        memcpy_buffer(dfr.back(), dev, a.data(), CPU_DEVICE, (size_t)a.size());
      }
      size_t i = 0;
      while (i < arrs.size()) {
        size_t j = i + 1;
        while (j < arrs.size() && arrs[j].shape(0) == arrs[i].shape(0) &&
               arrs[j].shape(1) == arrs[i].shape(1) &&
               arrs[j].shape(2) == arrs[i].shape(2))
          ++j;
        std::vector<const u8*> fp(dfr.begin() + i, dfr.begin() + j);
        png_encode_gpu(fp, (i32)arrs[i].shape(0), (i32)arrs[i].shape(1),
                       (i32)arrs[i].shape(2), dev, per_thread_hip_stream(),
                       bufs, sizes);
        i = j;
      }
      for (size_t k = 0; k < bufs.size(); ++k) {
        std::string host(sizes[k], '\0');
        memcpy_buffer((u8*)host.data(), CPU_DEVICE, bufs[k], dev, sizes[k]);
        res.append(py::bytes(host));
      }
    } catch (...) {
      cleanup();
      throw;
    }
    cleanup();
    return res;
  });
  // Seconds for `iters` encodes of `batch` device-resident h*w*c frames,
  // each ending with the files in host memory, and the bytes of one
  // iteration. mode "gpu": png_encode_gpu, then D2H of the files. mode
  // "cpu-parallel": D2H of the raw frames, then png_encode_parallel_cpu.
  // mode "zlib": D2H of the raw frames, then the zlib writer. The clips are
  // those of jpeg_encode_bench.
  m.def("png_encode_bench",
        [](i32 h, i32 w, i32 c, i64 batch, i32 iters, const std::string& mode,
           const std::string& clip) {
          SCA_CHECK(have_gpu(), "png_encode_bench needs a GPU");
          SCA_CHECK(mode == "gpu" || mode == "cpu-parallel" || mode == "zlib",
                    "mode must be 'gpu', 'cpu-parallel' or 'zlib'");
          SCA_CHECK(clip == "smooth" || clip == "noise",
                    "clip must be 'smooth' or 'noise'");
          png_check_args(h, w, c);
          SCA_CHECK(batch > 0 && iters > 0, "empty benchmark");
          size_t fsize = (size_t)h * w * c;
          DeviceHandle dev{DeviceType::GPU, 0};
          u8* d = new_block_buffer(dev, fsize * batch, 1);
          double secs = 0;
          u64 out_bytes = 0;
          try {
            {
              std::vector<u8> host(fsize * batch);
              u32 x = 2654435761u;
              size_t p = 0;
              for (i64 i = 0; i < batch; ++i)
                for (i32 y = 0; y < h; ++y)
                  for (i32 xx = 0; xx < w; ++xx)
                    for (i32 ch = 0; ch < c; ++ch, ++p) {
                      if (clip == "noise") {
                        x ^= x << 13; x ^= x >> 17; x ^= x << 5;
                        host[p] = (u8)(x >> 24);
                      } else {
                        i64 v = ch % 3 == 0   ? xx + i * 2
                                : ch % 3 == 1 ? y + i
                                              : (xx + y) / 2 + i * 3;
                        host[p] = (u8)(v & 0xff);
                      }
                    }
              memcpy_buffer(d, dev, host.data(), CPU_DEVICE, fsize * batch);
            }
            std::vector<const u8*> fp;
            for (i64 i = 0; i < batch; ++i) fp.push_back(d + (size_t)i * fsize);
            py::gil_scoped_release rel;
            auto t0 = std::chrono::steady_clock::now();
            for (i32 it = 0; it < iters; ++it) {
              out_bytes = 0;
              if (mode == "gpu") {
                std::vector<u8*> bufs;
                std::vector<u64> sizes;
                png_encode_gpu(fp, h, w, c, dev, per_thread_hip_stream(), bufs,
                               sizes);
                std::vector<u8*> dst;
                std::vector<const u8*> src(bufs.begin(), bufs.end());
                std::vector<size_t> sz(sizes.begin(), sizes.end());
                for (u64 s : sizes) {
                  dst.push_back(new_buffer(CPU_DEVICE, s));
                  out_bytes += s;
                }
                memcpy_vec(dst, CPU_DEVICE, src, dev, sz);
                for (u8* b : dst) delete_buffer(CPU_DEVICE, b);
                for (u8* b : bufs) delete_buffer(dev, b);
              } else {
                std::vector<u8*> dst;
                std::vector<size_t> sz(batch, fsize);
                for (i64 i = 0; i < batch; ++i)
                  dst.push_back(new_buffer(CPU_DEVICE, fsize));
                memcpy_vec(dst, CPU_DEVICE, fp, dev, sz);
                for (i64 i = 0; i < batch; ++i) {
                  auto v = mode == "zlib"
                               ? encode_png(dst[i], h, w, c)
                               : png_encode_parallel_cpu(dst[i], h, w, c);
                  out_bytes += v.size();
                  delete_buffer(CPU_DEVICE, dst[i]);
                }
              }
            }
            secs = std::chrono::duration<double>(
                       std::chrono::steady_clock::now() - t0)
                       .count();
          } catch (...) {
            delete_buffer(dev, d);
            throw;
          }
          delete_buffer(dev, d);
          return py::make_tuple(secs, out_bytes);
        },
        py::arg("h"), py::arg("w"), py::arg("c"), py::arg("batch") = 8,
        py::arg("iters") = 1, py::arg("mode") = "gpu",
        py::arg("clip") = "smooth");
  // ---- still-image decode (ops/jpeg_decode_cpu.cpp, ops/png_decode.cpp,
  // kernels/jpeg_decode.hip)
  auto image_to_array = [](const DecodedImage& img) {
    py::array_t<u8> a({(i64)img.h, (i64)img.w, (i64)img.c});
    std::memcpy(a.mutable_data(), img.pixels.data(), img.pixels.size());
    return a;
  };
  m.def("jpeg_decode_info", [](py::bytes blob, const std::string& progressive) {
    JpegParseOptions po;
    po.allow_progressive =
        jpeg_progressive_option(progressive, "jpeg_decode_info");
    std::string s = blob;
    JpegInfo in = jpeg_parse((const u8*)s.data(), s.size(), po);
    py::dict d;
    d["h"] = in.g.h;
    d["w"] = in.g.w;
    d["c"] = in.g.nc;
    d["hs"] = in.g.hs;
    d["vs"] = in.g.vs;
    d["mcus"] = in.g.nmcu;
    d["restart_interval"] = in.restart_interval;
    py::list segs;
    for (auto& sg : in.segments)
      segs.append(py::make_tuple(sg.begin, sg.end, sg.first_mcu,
                                 sg.mcu_count));
    d["segments"] = segs;
    d["progressive"] = in.progressive;
    py::list scans;
    for (auto& sc : in.scans) {
      py::dict e;
      py::list comps;
      for (u32 c = 0; c < sc.ncomp; ++c) comps.append(sc.comp[c]);
      e["components"] = comps;
      e["ss"] = sc.ss;
      e["se"] = sc.se;
      e["ah"] = sc.ah;
      e["al"] = sc.al;
      e["restart_interval"] = sc.restart_interval;
      e["units"] = sc.units;
      e["segment_count"] = sc.segments.size();
      py::list ssegs;
      for (auto& sg : sc.segments)
        ssegs.append(py::make_tuple(sg.begin, sg.end, sg.first_mcu,
                                    sg.mcu_count));
      e["segments"] = ssegs;
      scans.append(e);
    }
    d["scans"] = scans;
    return d;
  }, py::arg("blob"), py::arg("progressive") = "reject");
  // the oracle: file bytes -> [H,W,C] u8
  m.def("jpeg_cpu_decode", [image_to_array](py::bytes blob,
                                            const std::string& progressive) {
    JpegParseOptions po;
    po.allow_progressive =
        jpeg_progressive_option(progressive, "jpeg_cpu_decode");
    std::string s = blob;
    return image_to_array(jpeg_decode_cpu((const u8*)s.data(), s.size(), po));
  }, py::arg("blob"), py::arg("progressive") = "reject");
  // debug seam: the quantised coefficients of a baseline or progressive
  // file, per component as int16 [blocks_y, blocks_x, 64] in natural order
  // over the component's own raster, ceil(comp_w / 8) x ceil(comp_h / 8)
  m.def("jpeg_decode_coefficients", [](py::bytes blob,
                                       const std::string& progressive) {
    JpegParseOptions po;
    po.allow_progressive =
        jpeg_progressive_option(progressive, "jpeg_decode_coefficients");
    std::string s = blob;
    JpegInfo in = jpeg_parse((const u8*)s.data(), s.size(), po);
    std::vector<i16> coef;
    jpeg_coefficients_cpu((const u8*)s.data(), in, coef);
    py::list res;
    for (u32 c = 0; c < (u32)in.g.nc; ++c) {
      u32 bw, bh;
      jpeg_prog_comp_blocks(in.g, c, bw, bh);
      py::array_t<i16> a({(i64)bh, (i64)bw, (i64)64});
      i16* dst = a.mutable_data();
      for (u32 by = 0; by < bh; ++by)
        for (u32 bx = 0; bx < bw; ++bx)
          std::memcpy(dst + ((size_t)by * bw + bx) * 64,
                      coef.data() +
                          (size_t)jpeg_prog_block_index(in.g, c, bx, by) * 64,
                      128);
      res.append(a);
    }
    return res;
  }, py::arg("blob"), py::arg("progressive") = "reject");
  m.def("png_cpu_decode", [image_to_array](py::bytes blob) {
    std::string s = blob;
    return image_to_array(png_decode((const u8*)s.data(), s.size()));
  });
  m.def("image_cpu_decode", [image_to_array](py::bytes blob,
                                             const std::string& progressive) {
    JpegParseOptions po;
    po.allow_progressive =
        jpeg_progressive_option(progressive, "image_cpu_decode");
    std::string s = blob;
    return image_to_array(
        image_decode_cpu((const u8*)s.data(), s.size(), po));
  }, py::arg("blob"), py::arg("progressive") = "reject");
  // dequantised int32 blocks [N,64] (natural order; values are clamped to
  // the decoder's coefficient limit) -> u8 samples [N,64]
  m.def("jpeg_idct_blocks",
        [](py::array_t<i32, py::array::c_style | py::array::forcecast> blocks) {
          SCA_CHECK(blocks.ndim() == 2 && blocks.shape(1) == 64,
                    "blocks must be [N,64]");
          i64 n = blocks.shape(0);
          py::array_t<u8> out({n, (i64)64});
          const i32* src = blocks.data();
          u8* dst = out.mutable_data();
          for (i64 b = 0; b < n; ++b) {
            i32 deq[64];
            u8 pix[64];
            for (int k = 0; k < 64; ++k) {
              i32 v = src[b * 64 + k];
              deq[k] = v < -kJpegCoefLimit  ? -kJpegCoefLimit
                       : v > kJpegCoefLimit ? kJpegCoefLimit
                                            : v;
            }
            jpeg_idct_block(deq, pix);
            std::memcpy(dst + b * 64, pix, 64);
          }
          return out;
        });
  // The self-synchronising decoder's CPU model (ops/jpeg_sync_cpu.cpp) on a
  // JPEG without restart markers -> ([H,W,C] u8, stats dict). chunk_bytes 0
  // is the default, jpeg_sync_chunk_bytes().
  m.def("jpeg_sync_chunk_bytes", []() { return kJpegSyncChunkBytes; });
  m.def("jpeg_sync_model",
        [](py::bytes blob, u32 chunk_bytes) {
          std::string s = blob;
          JpegInfo in = jpeg_parse((const u8*)s.data(), s.size());
          py::array_t<u8> a({(i64)in.g.h, (i64)in.g.w, (i64)in.g.nc});
          JpegSyncStats st;
          jpeg_decode_sync_model((const u8*)s.data(), in, chunk_bytes,
                                 a.mutable_data(), &st);
          py::dict d;
          d["chunks"] = st.chunks;
          d["groups"] = st.groups;
          d["group_iterations"] = st.group_iterations;
          d["cross_rounds"] = st.cross_rounds;
          d["cross_repairs"] = st.cross_repairs;
          d["stuffed_starts"] = st.stuffed_starts;
          d["empty_chunks"] = st.empty_chunks;
          d["status"] = st.status;
          d["verified"] = st.verified;
          d["fallback"] = !st.verified;
          return py::make_tuple(a, d);
        },
        py::arg("blob"), py::arg("chunk_bytes") = 0);
  // One batch through jpeg_decode_gpu -> list of [H,W,C] u8 arrays, in
  // order; with host_rows=True also the number of rows the CPU decoders
  // handled (PNG; JPEG without DRI unless serial_scan="device", and then
  // those that failed verification); with stats=True also a dict of the
  // self-synchronising decoder's row counts. progressive="decode" allows
  // progressive files (image_decode.h says which go to the device) and adds
  // their device row count to that dict.
  m.def("jpeg_gpu_decode",
        [](const std::vector<py::bytes>& blobs, bool want_host_rows,
           const std::string& serial_scan, u32 chunk_bytes, bool want_stats,
           const std::string& progressive) -> py::object {
          JpegParseOptions po;
          po.allow_progressive =
              jpeg_progressive_option(progressive, "jpeg_gpu_decode");
          SCA_CHECK(have_gpu(), "jpeg_gpu_decode needs a GPU");
          SCA_CHECK(serial_scan == "host" || serial_scan == "device",
                    "serial_scan must be 'host' or 'device', got '" +
                        serial_scan + "'");
          JpegGpuOptions opt;
          opt.progressive = po.allow_progressive;
          opt.serial_scan_on_device = serial_scan == "device";
          opt.chunk_bytes = chunk_bytes;
          DeviceHandle dev{DeviceType::GPU, 0};
          std::vector<std::string> data(blobs.begin(), blobs.end());
          std::vector<ImageBlob> ib;
          std::vector<JpegInfo> infos(data.size());
          for (size_t i = 0; i < data.size(); ++i) {
            ib.push_back({(const u8*)data[i].data(), data[i].size()});
            if (is_jpeg(ib[i].data, ib[i].size)) {
              try {
                infos[i] = jpeg_parse(ib[i].data, ib[i].size, po);
              } catch (const ScannerError& err) {
                throw ScannerError("ImageDecoder: row " + std::to_string(i) +
                                   " of the batch: " + err.what());
              }
            }
          }
          std::vector<DeviceFrame> frames;
          i64 host_rows = 0;
          JpegGpuStats gs;
          jpeg_decode_gpu(ib, infos, dev, per_thread_hip_stream(), frames,
                          &host_rows, opt, &gs);
          py::list res;
          try {
            for (auto& f : frames) {
              py::array_t<u8> a({(i64)f.h, (i64)f.w, (i64)f.c});
              memcpy_buffer(a.mutable_data(), CPU_DEVICE, f.buffer, dev,
                            (size_t)f.h * f.w * f.c);
              res.append(a);
            }
          } catch (...) {
            for (auto& f : frames) delete_buffer(dev, f.buffer);
            throw;
          }
          for (auto& f : frames) delete_buffer(dev, f.buffer);
          py::dict sd;
          sd["sync_rows"] = gs.sync_rows;
          sd["fallback_rows"] = gs.fallback_rows;
          // only on request: the dict of a default call is what it was
          if (po.allow_progressive)
            sd["progressive_rows"] = gs.progressive_rows;
          if (want_host_rows && want_stats)
            return py::make_tuple(res, host_rows, sd);
          if (want_host_rows) return py::make_tuple(res, host_rows);
          if (want_stats) return py::make_tuple(res, sd);
          return std::move(res);
        },
        py::arg("blobs"), py::arg("host_rows") = false,
        py::arg("serial_scan") = "host", py::arg("chunk_bytes") = 0,
        py::arg("stats") = false, py::arg("progressive") = "reject");
  // Seconds of each of `iters` decodes of the batch, every one ending with
  // the frames resident in HBM. mode "gpu": jpeg_parse + jpeg_decode_gpu
  // (compressed H2D inside; serial_scan and chunk_bytes as for
  // jpeg_gpu_decode). mode "cpu": jpeg_decode_cpu on this thread,
  // then H2D of the raw frames. mode "upload": the blobs are raw pixels
  // already (another decoder's output); one host copy and the H2D.
  m.def("jpeg_decode_bench",
        [](const std::vector<py::bytes>& blobs, i32 iters,
           const std::string& mode, const std::string& serial_scan,
           u32 chunk_bytes, const std::string& progressive) {
          JpegParseOptions po;
          po.allow_progressive =
              jpeg_progressive_option(progressive, "jpeg_decode_bench");
          SCA_CHECK(have_gpu(), "jpeg_decode_bench needs a GPU");
          SCA_CHECK(serial_scan == "host" || serial_scan == "device",
                    "serial_scan must be 'host' or 'device', got '" +
                        serial_scan + "'");
          JpegGpuOptions opt;
          opt.serial_scan_on_device = serial_scan == "device";
          opt.chunk_bytes = chunk_bytes;
          opt.progressive = po.allow_progressive;
          SCA_CHECK(mode == "gpu" || mode == "cpu" || mode == "upload",
                    "mode must be 'gpu', 'cpu' or 'upload'");
          SCA_CHECK(!blobs.empty() && iters > 0, "empty benchmark");
          DeviceHandle dev{DeviceType::GPU, 0};
          std::vector<std::string> data(blobs.begin(), blobs.end());
          std::vector<double> secs;
          py::gil_scoped_release rel;
          for (i32 it = 0; it < iters; ++it) {
            auto t0 = std::chrono::steady_clock::now();
            if (mode == "gpu") {
              std::vector<ImageBlob> ib;
              std::vector<JpegInfo> infos(data.size());
              for (size_t i = 0; i < data.size(); ++i) {
                ib.push_back({(const u8*)data[i].data(), data[i].size()});
                infos[i] = jpeg_parse(ib[i].data, ib[i].size, po);
              }
              std::vector<DeviceFrame> frames;
              jpeg_decode_gpu(ib, infos, dev, per_thread_hip_stream(),
                              frames, nullptr, opt);
              secs.push_back(std::chrono::duration<double>(
                                 std::chrono::steady_clock::now() - t0)
                                 .count());
              for (auto& f : frames) delete_buffer(dev, f.buffer);
            } else {
              std::vector<DecodedImage> imgs;
              size_t total = 0;
              for (auto& d : data) {
                if (mode == "upload") {  // the blobs are decoded pixels
                  imgs.emplace_back();
                  imgs.back().pixels.assign(d.begin(), d.end());
                } else {
                  imgs.push_back(
                      jpeg_decode_cpu((const u8*)d.data(), d.size(), po));
                }
                total += (imgs.back().pixels.size() + 255) / 256 * 256;
              }
              u8* block = new_block_buffer(dev, total, 1);
              std::vector<u8*> dst;
              std::vector<const u8*> src;
              std::vector<size_t> sz;
              size_t pos = 0;
              for (auto& im : imgs) {
                dst.push_back(block + pos);
                src.push_back(im.pixels.data());
                sz.push_back(im.pixels.size());
                pos += (im.pixels.size() + 255) / 256 * 256;
              }
              memcpy_vec(dst, dev, src, CPU_DEVICE, sz);
              secs.push_back(std::chrono::duration<double>(
                                 std::chrono::steady_clock::now() - t0)
                                 .count());
              delete_buffer(dev, block);
            }
          }
          return secs;
        },
        py::arg("blobs"), py::arg("iters") = 1, py::arg("mode") = "gpu",
        py::arg("serial_scan") = "host", py::arg("chunk_bytes") = 0,
        py::arg("progressive") = "reject");
  // seconds the calling thread's last jpeg_decode_gpu waited in its stream
  // synchronise (the rest of the call is host work: parse, pack, enqueue)
  m.def("jpeg_decode_last_sync_seconds", &jpeg_decode_gpu_last_sync_seconds);
  m.def("span_cache_clear", &span_cache_clear);
  m.def("span_cache_set_budget", &span_cache_set_budget);
  // engine memory accounting (device -1 = CPU)
  m.def("mem_stats", [](int device) {
    DeviceHandle d = device < 0 ? CPU_DEVICE
                                : DeviceHandle{DeviceType::GPU, device};
    py::dict r;
    r["live"] = mem_bytes_live(d);
    r["peak"] = mem_bytes_peak(d);
    return r;
  });
  m.def("mem_reset_peak", [](int device) {
    DeviceHandle d = device < 0 ? CPU_DEVICE
                                : DeviceHandle{DeviceType::GPU, device};
    mem_reset_peak(d);
  });

  m.def("registered_ops", [] { return op_registry().names(); });
  m.def("registered_sources", [] { return source_registry().names(); });
  m.def("registered_sinks", [] { return sink_registry().names(); });
  m.def("op_info", [](const std::string& name) {
    const OpInfo& o = op_registry().get(name);
    py::dict d;
    py::list ins, outs;
    for (auto& c : o.input_columns)
      ins.append(py::make_tuple(c.name, (i32)c.type));
    for (auto& c : o.output_columns)
      outs.append(py::make_tuple(c.name, (i32)c.type));
    d["input_columns"] = ins;
    d["output_columns"] = outs;
    d["variadic"] = o.variadic_inputs;
    d["stencil"] = o.stencil;
    d["bounded_state"] = o.has_bounded_state;
    d["warmup"] = o.warmup;
    d["unbounded_state"] = o.has_unbounded_state;
    return d;
  });
  m.def("has_kernel", [](const std::string& op, i32 device) {
    return kernel_registry().has(op, (DeviceType)device);
  });
  // One registered kernel, one execute() call, on inputs the caller shapes
  // (tests/test_image_ops_*.py). `frames` are equal-shape u8 HWC arrays, or
  // f32 H x W x 2 flow arrays. packed: all frames end to end in ONE block
  // buffer without padding, so odd frame sizes sit at odd addresses as
  // decoded frames do; otherwise one allocation per frame. Row i sees the
  // elements i + stencil[j] (the same Element for every row that names it),
  // so n + max(stencil) frames make n rows. Returns column 0 per row: frames
  // as arrays shaped by their frame_info, blobs as bytes. With then_op, a
  // second kernel runs on those outputs without leaving the device and the
  // result is (first outputs, second outputs).
  m.def(
      "op_kernel_test",
      [](const std::string& op, i32 device_type, const py::bytes& args_b,
         const std::vector<py::array>& frames, const std::vector<i32>& stencil,
         bool packed, const std::string& then_op,
         const py::bytes& then_args_b) -> py::object {
        SCA_CHECK(device_type == 0 || device_type == 1,
                  "op_kernel_test: bad device type");
        const bool gpu = device_type == (i32)DeviceType::GPU;
        SCA_CHECK(!gpu || have_gpu(), "op_kernel_test needs a GPU");
        const DeviceHandle dev = gpu ? kTestDev : CPU_DEVICE;
        SCA_CHECK(!frames.empty(), "op_kernel_test: no frames");
        SCA_CHECK(!stencil.empty() && stencil[0] == 0,
                  "op_kernel_test: stencil must start at 0");
        i32 reach = 0;
        for (i32 s : stencil) {
          SCA_CHECK(s >= 0, "op_kernel_test: negative stencil offset");
          reach = std::max(reach, s);
        }
        SCA_CHECK((size_t)reach < frames.size(),
                  "op_kernel_test: fewer frames than the stencil spans");
        const size_t nrows = frames.size() - reach;

        // host side: contiguous copies, one geometry
        const bool is_f32 = py::isinstance<py::array_t<float>>(frames[0]);
        SCA_CHECK(is_f32 || py::isinstance<py::array_t<u8>>(frames[0]),
                  "op_kernel_test: frames must be uint8 or float32");
        SCA_CHECK(frames[0].ndim() == 3, "op_kernel_test: frames must be 3-D");
        FrameInfo fi;
        for (int d = 0; d < 3; ++d) fi.shape[d] = (i32)frames[0].shape(d);
        fi.type = is_f32 ? FrameType::F32 : FrameType::U8;
        const size_t fbytes = fi.size();
        std::vector<py::array> host;
        for (const py::array& a : frames) {
          SCA_CHECK((is_f32 ? py::isinstance<py::array_t<float>>(a)
                            : py::isinstance<py::array_t<u8>>(a)) &&
                        a.ndim() == 3 &&
                        a.shape(0) == fi.shape[0] &&
                        a.shape(1) == fi.shape[1] && a.shape(2) == fi.shape[2],
                    "op_kernel_test: frames differ in shape or type");
          host.push_back(py::array::ensure(a, py::array::c_style));
          SCA_CHECK(host.back() && (size_t)host.back().nbytes() == fbytes,
                    "op_kernel_test: frame is not contiguous");
        }

        // Everything allocated here or by the kernel is released on every
        // way out, a rejected input included.
        struct Owned {
          std::vector<Element> elems;
          ~Owned() {
            for (Element& e : elems)
              if (e.buffer) delete_buffer(e.device, e.buffer);
          }
        } inputs, outputs;
        u8* block = nullptr;
        if (packed)
          block = new_block_buffer(dev, fbytes * host.size(),
                                   (i32)host.size());
        for (size_t i = 0; i < host.size(); ++i) {
          Element e;
          e.is_frame = true;
          e.frame_info = fi;
          e.size = fbytes;
          e.device = dev;
          e.index = (i64)i;
          e.buffer = packed ? block + i * fbytes : new_buffer(dev, fbytes);
          inputs.elems.push_back(e);
        }
        for (size_t i = 0; i < host.size(); ++i)
          memcpy_buffer(inputs.elems[i].buffer, dev,
                        (const u8*)host[i].data(), CPU_DEVICE, fbytes);

        // one execute() of a registered kernel over `nr` rows; the outputs
        // of every column go to `outputs` (owned), column 0 is returned
        auto run = [&](const std::string& name, const std::string& args,
                       const StenciledElements& in, size_t nr) {
          const KernelFactory& f =
              kernel_registry().get(name, (DeviceType)device_type);
          KernelConfig cfg;
          cfg.device = dev;
          cfg.output_device = dev;
          if (f.output_device_type >= 0)
            cfg.output_device = f.output_device_type == (i32)DeviceType::GPU
                                    ? kTestDev
                                    : CPU_DEVICE;
          const OpInfo& info = op_registry().get(name);
          for (auto& c : info.input_columns)
            cfg.input_columns.push_back(c.name);
          for (auto& c : info.output_columns)
            cfg.output_columns.push_back(c.name);
          cfg.args.assign(args.begin(), args.end());
          cfg.max_batch = (i32)nr;
          cfg.hip_stream = gpu ? per_thread_hip_stream() : nullptr;
          std::unique_ptr<BaseKernel> kernel = f.make(cfg);
          BatchedElements out(
              std::max<size_t>(1, info.output_columns.size()));
          try {
            kernel->execute(in, out);
          } catch (...) {
            for (auto& col : out)
              for (Element& e : col) outputs.elems.push_back(e);
            if (gpu) sync_per_thread_stream();
            throw;
          }
          for (auto& col : out)
            for (Element& e : col) {
              if (!e.is_null && e.buffer) e.device = cfg.output_device;
              outputs.elems.push_back(e);
            }
          if (gpu) sync_per_thread_stream();
          SCA_CHECK(out[0].size() == nr,
                    "op_kernel_test: " + name + " returned " +
                        std::to_string(out[0].size()) + " rows for " +
                        std::to_string(nr));
          return out[0];
        };
        auto download = [](const ElementVector& col) {
          py::list res;
          for (const Element& e : col) {
            if (e.is_frame) {
              SCA_CHECK(e.frame_info.size() == e.size,
                        "op_kernel_test: frame_info disagrees with size");
              std::vector<py::ssize_t> shape = {e.frame_info.shape[0],
                                                e.frame_info.shape[1],
                                                e.frame_info.shape[2]};
              py::array a;
              if (e.frame_info.type == FrameType::F32)
                a = py::array_t<float>(shape);
              else if (e.frame_info.type == FrameType::U8)
                a = py::array_t<u8>(shape);
              else
                throw ScannerError("op_kernel_test: unsupported output type");
              memcpy_buffer((u8*)a.mutable_data(), CPU_DEVICE, e.buffer,
                            e.device, e.size);
              res.append(a);
            } else {
              std::string blob(e.size, '\0');
              memcpy_buffer((u8*)blob.data(), CPU_DEVICE, e.buffer, e.device,
                            e.size);
              res.append(py::bytes(blob));
            }
          }
          return res;
        };

        StenciledElements in(1);
        in[0].resize(nrows);
        for (size_t r = 0; r < nrows; ++r)
          for (i32 s : stencil) in[0][r].push_back(inputs.elems[r + s]);
        ElementVector first = run(op, std::string(args_b), in, nrows);
        if (then_op.empty()) return py::object(download(first));
        // the first kernel's outputs stay where they are and feed a second
        // kernel (stencil [0]), as two ops of one graph on one device do
        StenciledElements in2(1);
        in2[0].resize(nrows);
        for (size_t r = 0; r < nrows; ++r) in2[0][r].push_back(first[r]);
        ElementVector second = run(then_op, std::string(then_args_b), in2, nrows);
        return py::object(py::make_tuple(download(first), download(second)));
      },
      py::arg("op_name"), py::arg("device_type"), py::arg("args_bytes"),
      py::arg("frames"), py::arg("stencil") = std::vector<i32>{0},
      py::arg("packed") = true, py::arg("then_op") = "",
      py::arg("then_args") = py::bytes());
  // Seconds for `iters` execute() calls of ONE Resize kernel object on
  // `batch` resident sh x sw x c noise frames (tools/bench_resize.py): the
  // steady state of a pipeline instance, tables and workspace cached. On
  // the GPU the clock stops after the stream has drained.
  m.def(
      "resize_bench",
      [](i32 device_type, const py::bytes& args_b, i32 sh, i32 sw, i32 c,
         i32 batch, i32 iters) {
        SCA_CHECK(device_type == 0 || device_type == 1,
                  "resize_bench: bad device type");
        const bool gpu = device_type == (i32)DeviceType::GPU;
        SCA_CHECK(!gpu || have_gpu(), "resize_bench needs a GPU");
        SCA_CHECK(sh > 0 && sw > 0 && c > 0 && batch > 0 && iters > 0,
                  "resize_bench: empty benchmark");
        const DeviceHandle dev = gpu ? kTestDev : CPU_DEVICE;
        const size_t fsize = (size_t)sh * sw * c;
        u8* block = new_block_buffer(dev, fsize * batch, 1);
        double secs = 0;
        try {
          {
            std::vector<u8> host(fsize * batch);
            u32 x = 2654435761u;
            for (u8& b : host) {
              x ^= x << 13; x ^= x >> 17; x ^= x << 5;
              b = (u8)(x >> 24);
            }
            memcpy_buffer(block, dev, host.data(), CPU_DEVICE, host.size());
          }
          const KernelFactory& f =
              kernel_registry().get("Resize", (DeviceType)device_type);
          KernelConfig cfg;
          cfg.device = dev;
          cfg.output_device = dev;
          cfg.input_columns = {"frame"};
          cfg.output_columns = {"frame"};
          std::string args(args_b);
          cfg.args.assign(args.begin(), args.end());
          cfg.max_batch = batch;
          cfg.hip_stream = gpu ? per_thread_hip_stream() : nullptr;
          std::unique_ptr<BaseKernel> kernel = f.make(cfg);
          StenciledElements in(1);
          in[0].resize(batch);
          for (i32 i = 0; i < batch; ++i) {
            Element e;
            e.is_frame = true;
            e.frame_info.shape[0] = sh;
            e.frame_info.shape[1] = sw;
            e.frame_info.shape[2] = c;
            e.frame_info.type = FrameType::U8;
            e.size = fsize;
            e.device = dev;
            e.index = i;
            e.buffer = block + (size_t)i * fsize;
            in[0][i].push_back(e);
          }
          py::gil_scoped_release rel;
          auto once = [&] {
            BatchedElements out(1);
            try {
              kernel->execute(in, out);
            } catch (...) {
              if (gpu) sync_per_thread_stream();
              for (Element& e : out[0])
                if (e.buffer) delete_buffer(e.device, e.buffer);
              throw;
            }
            // an output goes back to the pool only once its kernel is done
            if (gpu) sync_per_thread_stream();
            for (Element& e : out[0])
              if (e.buffer) delete_buffer(e.device, e.buffer);
          };
          once();  // tables, workspace
          auto t0 = std::chrono::steady_clock::now();
          for (i32 it = 0; it < iters; ++it) once();
          secs = std::chrono::duration<double>(
                     std::chrono::steady_clock::now() - t0)
                     .count();
        } catch (...) {
          delete_buffer(dev, block);
          throw;
        }
        delete_buffer(dev, block);
        return secs;
      },
      py::arg("device_type"), py::arg("args_bytes"), py::arg("sh"),
      py::arg("sw"), py::arg("c") = 3, py::arg("batch") = 16,
      py::arg("iters") = 1);
  m.def("register_python_op", &register_python_op_binding);

  py::class_<Database, std::shared_ptr<Database>>(m, "Database")
      .def(py::init([](const std::string& path) {
        return std::make_shared<Database>(StorageBackend::make_posix(), path);
      }))
      .def(py::init([](const std::string& path,
                       const std::string& storage_type,
                       const std::string& bucket) {
        std::unique_ptr<StorageBackend> s;
        if (storage_type == "posix") {
          s = StorageBackend::make_posix();
        } else if (storage_type == "s3" || storage_type == "gcs" ||
                   storage_type == "object") {
          SCA_CHECK(!bucket.empty(),
                    "object storage needs a bucket path");
          s = StorageBackend::make_object_store(bucket);
        } else {
          throw ScannerError("unknown storage type '" + storage_type + "'");
        }
        return std::make_shared<Database>(std::move(s), path);
      }))
      .def("recover", &Database::recover)
      .def("write_megafile", &Database::write_megafile)
      .def("table_names", &Database::table_names)
      .def("has_table", &Database::has_table)
      .def("delete_table", &Database::delete_table)
      .def("table_committed",
           [](Database& db, const std::string& name) {
             return db.table_committed(db.get_table(name).id);
           })
      .def("table_info", [](Database& db, const std::string& name) {
        TableMetadata t = db.get_table(name);
        py::dict d;
        d["id"] = t.id;
        d["name"] = t.name;
        d["num_rows"] = t.num_rows();
        py::list cols;
        for (auto& c : t.columns)
          cols.append(py::make_tuple(c.name, (i32)c.type));
        d["columns"] = cols;
        d["end_rows"] = t.end_rows;
        d["committed"] = db.table_committed(t.id);
        return d;
      });

  // ---- table write/read helpers (client-side ingest + load) ----

  m.def("write_bytes_table",
        [](std::shared_ptr<Database> db, const std::string& name,
           const std::vector<std::string>& columns,
           const std::vector<std::vector<py::bytes>>& rows_per_column,
           i64 io_packet_size) {
          std::vector<ColumnType> types(columns.size(), ColumnType::Bytes);
          TableMetadata t = db->new_table(name, columns, types, true);
          i64 n = rows_per_column.empty() ? 0 : (i64)rows_per_column[0].size();
          std::vector<i64> ends;
          i32 item = 0;
          for (i64 s = 0; s < n; s += io_packet_size, ++item) {
            i64 e = std::min(n, s + io_packet_size);
            for (size_t c = 0; c < columns.size(); ++c) {
              std::vector<Element> elems;
              std::vector<std::string> bufs;
              for (i64 r = s; r < e; ++r) {
                bufs.push_back(rows_per_column[c][r]);
              }
              for (auto& bstr : bufs) {
                Element el;
                el.buffer = reinterpret_cast<u8*>(bstr.data());
                el.size = bstr.size();
                elems.push_back(el);
              }
              write_column_item(*db, t, columns[c], item, elems);
            }
            ends.push_back(e);
          }
          if (ends.empty()) ends.push_back(0);
          t.end_rows = ends;
          db->update_table(t);
          db->commit_table(t.id);
        });

  // ---- real-video ingest (mp4/Annex-B -> indexed h264 table) ----
  m.def("ingest_video_file",
        [](std::shared_ptr<Database> db, const std::string& name,
           const std::string& column, const std::string& path) {
          IngestResult r = ingest_video_file(*db, name, column, path);
          py::dict d;
          d["num_frames"] = r.num_frames;
          d["width"] = r.width;
          d["height"] = r.height;
          d["codec"] = r.codec;
          return d;
        });
  m.def("export_mp4",
        [](std::shared_ptr<Database> db, const std::string& name,
           const std::string& column, const std::string& path, double fps) {
          export_mp4(*db, name, column, path, fps);
        });
  // parser introspection (unit tests)
  m.def("h264_index", [](py::bytes b) {
    std::string s = b;
    H264Index idx = h264_index_annexb((const u8*)s.data(), s.size());
    py::dict d;
    d["width"] = idx.width;
    d["height"] = idx.height;
    d["num_frames"] = idx.num_frames;
    d["sample_offsets"] = idx.sample_offsets;
    d["sample_sizes"] = idx.sample_sizes;
    d["keyframe_indices"] = idx.keyframe_indices;
    d["sps"] = py::bytes((const char*)idx.sps.data(), idx.sps.size());
    d["pps"] = py::bytes((const char*)idx.pps.data(), idx.pps.size());
    return d;
  });
  m.def("mp4_probe", [](py::bytes b) {
    std::string s = b;
    Mp4Track t = mp4_parse((const u8*)s.data(), s.size());
    py::dict d;
    d["codec"] = t.codec;
    d["width"] = t.width;
    d["height"] = t.height;
    d["length_size"] = t.length_size;
    d["sample_offsets"] = t.sample_offsets;
    d["sample_sizes"] = t.sample_sizes;
    d["keyframe_indices"] = t.keyframe_indices;
    d["timescale"] = t.timescale;
    d["n_sps"] = (i64)t.sps.size();
    d["n_pps"] = (i64)t.pps.size();
    return d;
  });
  m.def("h264_parse_sps_py", [](py::bytes b) {
    std::string s = b;
    H264Sps sps = h264_parse_sps((const u8*)s.data(), s.size());
    py::dict d;
    d["width"] = sps.width;
    d["height"] = sps.height;
    d["profile_idc"] = sps.profile_idc;
    return d;
  });

  m.def("write_video_table",
        [](std::shared_ptr<Database> db, const std::string& name,
           const std::string& column,
           py::array_t<u8, py::array::c_style | py::array::forcecast> frames,
           i64 io_packet_size, const std::string& codec, i32 quality,
           const std::string& subsampling) {
          SCA_CHECK(frames.ndim() == 4, "frames must be [N,H,W,C] u8");
          MjpegOptions mjpeg_opt;
          if (codec == "mjpeg") {
            mjpeg_opt.quality = quality;
            mjpeg_opt.subsampling = jpeg_parse_subsampling(subsampling);
            jpeg_check_args((i32)frames.shape(1), (i32)frames.shape(2),
                            (i32)frames.shape(3), quality);
          }
          i64 n = frames.shape(0);
          i32 h = (i32)frames.shape(1), w = (i32)frames.shape(2),
              c = (i32)frames.shape(3);
          size_t fsize = (size_t)h * w * c;
          TableMetadata t =
              db->new_table(name, {column}, {ColumnType::Video}, true);
          const u8* data = frames.data();
          std::vector<i64> ends;
          i32 item = 0;
          for (i64 s = 0; s < n; s += io_packet_size, ++item) {
            i64 e = std::min(n, s + io_packet_size);
            VideoMetadata vm;
            vm.width = w;
            vm.height = h;
            vm.channels = c;
            vm.frame_type = FrameType::U8;
            vm.num_frames = e - s;
            if (codec == "raw") {
              vm.codec = "raw";
              std::vector<Element> elems;
              for (i64 r = s; r < e; ++r) {
                Element el;
                el.buffer = const_cast<u8*>(data + (size_t)r * fsize);
                el.size = fsize;
                elems.push_back(el);
              }
              write_column_item(*db, t, column, item, elems);
              for (i64 r = s; r < e; ++r) {
                vm.keyframe_indices.push_back(r - s);
                vm.sample_offsets.push_back((r - s) * fsize);
                vm.sample_sizes.push_back(fsize);
              }
              auto vbuf = vm.serialize();
              db->storage()->write_all(
                  db->paths().video_metadata(t.id, t.column_id(column), item),
                  vbuf.data(), vbuf.size());
            } else if (codec == "svc") {
              std::vector<u8> stream;
              svc_encode_cpu(data + (size_t)s * fsize, e - s, h, w, c,
                             /*gop=*/16, stream, vm);
              write_video_item(*db, t, column, item, stream, vm);
            } else if (codec == "mjpeg") {
              std::vector<u8> stream;
              mjpeg_encode_cpu(data + (size_t)s * fsize, e - s, h, w, c,
                               mjpeg_opt, stream, vm);
              write_video_item(*db, t, column, item, stream, vm);
            } else {
              throw ScannerError("unknown codec '" + codec + "'");
            }
            ends.push_back(e);
          }
          if (ends.empty()) ends.push_back(0);
          t.end_rows = ends;
          db->update_table(t);
          db->commit_table(t.id);
        },
        py::arg("db"), py::arg("name"), py::arg("column"), py::arg("frames"),
        py::arg("io_packet_size") = 128, py::arg("codec") = "raw",
        py::arg("quality") = 90,
        py::arg("subsampling") = kMjpegDefaultSubsampling);

  // ---- Motion-JPEG (video/mjpeg.h, kernels/mjpeg_index.hip) ----
  // The restart-segment index of samples [offsets[i], +sizes[i]) of
  // `stream`. The reference header is the first header_len bytes of sample
  // 0; its geometry and restart interval give the MCUs per segment, nseg is
  // the caller's. Returns (segments [n, nseg, 4] u32, status [n] u32);
  // segments are offsets into `stream` and zero for a sample with a status.
  auto mjpeg_index_setup = [](const std::string& s,
                              const std::vector<u64>& offsets,
                              const std::vector<u64>& sizes, u32 header_len,
                              u32 nseg, MjpegIndexParams& p) {
    SCA_CHECK(!offsets.empty() && offsets.size() == sizes.size(),
              "one size per offset, at least one sample");
    for (size_t i = 0; i < offsets.size(); ++i)
      SCA_CHECK(offsets[i] <= s.size() && sizes[i] <= s.size() - offsets[i],
                "sample " + std::to_string(i) + " lies outside the stream");
    SCA_CHECK(header_len <= sizes[0], "header_len exceeds sample 0");
    SCA_CHECK(nseg >= 1, "nseg must be at least 1");
    auto ref =
        mjpeg_ref_header((const u8*)s.data() + offsets[0], sizes[0]);
    SCA_CHECK(ref->params.header_len == header_len,
              "header_len is not where the scan of sample 0 starts (" +
                  std::to_string(ref->params.header_len) + ")");
    p = ref->params;
    p.nseg = nseg;
  };
  auto mjpeg_index_result = [](const std::vector<MjpegSeg>& segs,
                               const std::vector<u32>& status, u32 nseg) {
    py::array_t<u32> sa({(i64)status.size(), (i64)nseg, (i64)4});
    std::memcpy(sa.mutable_data(), segs.data(), segs.size() * sizeof(MjpegSeg));
    py::array_t<u32> st({(i64)status.size()});
    std::memcpy(st.mutable_data(), status.data(), status.size() * 4);
    return py::make_tuple(sa, st);
  };
  m.def("mjpeg_index_ref",
        [mjpeg_index_setup, mjpeg_index_result](
            py::bytes stream, std::vector<u64> offsets, std::vector<u64> sizes,
            u32 header_len, u32 nseg) {
          std::string s = stream;
          MjpegIndexParams p;
          mjpeg_index_setup(s, offsets, sizes, header_len, nseg, p);
          const u8* ref = (const u8*)s.data() + offsets[0];
          size_t n = offsets.size();
          std::vector<MjpegSeg> segs(n * nseg, MjpegSeg{0, 0, 0, 0});
          std::vector<u32> status(n, 0);
          for (size_t i = 0; i < n; ++i) {
            status[i] = mjpeg_index_ref((const u8*)s.data() + offsets[i],
                                        sizes[i], ref, p, (u32)offsets[i],
                                        segs.data() + i * nseg);
            if (status[i] != kMjpegOk)
              std::fill(segs.begin() + i * nseg, segs.begin() + (i + 1) * nseg,
                        MjpegSeg{0, 0, 0, 0});
          }
          return mjpeg_index_result(segs, status, nseg);
        },
        py::arg("stream"), py::arg("offsets"), py::arg("sizes"),
        py::arg("header_len"), py::arg("nseg"));
  m.def("mjpeg_index_gpu",
        [mjpeg_index_setup, mjpeg_index_result](
            py::bytes stream, std::vector<u64> offsets, std::vector<u64> sizes,
            u32 header_len, u32 nseg) {
          SCA_CHECK(have_gpu(), "mjpeg_index_gpu needs a GPU");
          std::string s = stream;
          MjpegIndexParams p;
          mjpeg_index_setup(s, offsets, sizes, header_len, nseg, p);
          std::vector<MjpegSeg> segs;
          std::vector<u32> status;
          mjpeg_index_gpu((const u8*)s.data(), s.size(), offsets, sizes,
                          (const u8*)s.data() + offsets[0], p, segs, status);
          return mjpeg_index_result(segs, status, nseg);
        },
        py::arg("stream"), py::arg("offsets"), py::arg("sizes"),
        py::arg("header_len"), py::arg("nseg"));
  // Header length, segment count and restart interval of a JPEG file, as
  // the codec derives them from a reference header.
  m.def("mjpeg_header_info", [](py::bytes blob) {
    std::string s = blob;
    auto ref = mjpeg_ref_header((const u8*)s.data(), s.size());
    py::dict d;
    d["header_len"] = ref->params.header_len;
    d["nseg"] = ref->params.nseg;
    d["mcus_per_seg"] = ref->params.mcus_per_seg;
    d["nmcu"] = ref->params.nmcu;
    d["has_dri"] = ref->device_ok;
    return d;
  });
  // Timing of the two GPU decode paths of an mjpeg stream (tools/
  // bench_mjpeg.py): "index" decodes from a device-resident copy with the
  // device-side index (mjpeg_decode_gpu_dev); "host" is the still-image
  // path, jpeg_parse of every sample on the host and jpeg_decode_gpu, which
  // uploads the entropy bytes; "index_kernel" is the index kernel alone.
  // The modes alternate window by window in this one process, each window
  // ends synchronised, the first `warmup` windows of each are dropped.
  // Returns {mode: [seconds per window]}.
  m.def("mjpeg_decode_bench",
        [](py::bytes stream, std::vector<u64> offsets, std::vector<u64> sizes,
           i32 h, i32 w, i32 c, int windows, int warmup) {
          SCA_CHECK(have_gpu(), "mjpeg_decode_bench needs a GPU");
          std::string s = stream;
          size_t n = offsets.size();
          SCA_CHECK(n > 0 && sizes.size() == n, "one size per offset");
          VideoMetadata vm;
          vm.codec = "mjpeg";
          vm.height = h;
          vm.width = w;
          vm.channels = c;
          vm.num_frames = (i64)n;
          vm.sample_offsets = offsets;
          vm.sample_sizes = sizes;
          std::vector<i64> want;
          for (size_t i = 0; i < n; ++i) {
            SCA_CHECK(offsets[i] <= s.size() &&
                          sizes[i] <= s.size() - offsets[i],
                      "sample " + std::to_string(i) +
                          " lies outside the stream");
            want.push_back((i64)i);
          }
          const u8* base = (const u8*)s.data();
          auto ref = mjpeg_ref_header(base + offsets[0], sizes[0]);
          DeviceHandle dev{DeviceType::GPU, 0};
          u8* d = new_buffer(dev, s.size());
          std::vector<double> t_index, t_host, t_kernel;
          try {
            memcpy_buffer(d, dev, base, CPU_DEVICE, s.size());
            auto now = [] { return std::chrono::steady_clock::now(); };
            auto secs = [](auto a, auto b) {
              return std::chrono::duration<double>(b - a).count();
            };
            for (int it = 0; it < windows + warmup; ++it) {
              auto t0 = now();
              MjpegGpuStats st;
              auto elems =
                  mjpeg_decode_gpu_dev(d, 0, vm, want, dev, *ref, &st);
              auto t1 = now();
              for (auto& e : elems) delete_buffer(dev, e.buffer);
              SCA_CHECK(st.fallback_frames == 0,
                        "mjpeg_decode_bench: frames fell back");
              auto t2 = now();
              std::vector<ImageBlob> blobs(n);
              std::vector<JpegInfo> infos(n);
              for (size_t i = 0; i < n; ++i) {
                blobs[i] = {base + offsets[i], (size_t)sizes[i]};
                infos[i] = jpeg_parse(blobs[i].data, blobs[i].size);
              }
              std::vector<DeviceFrame> frames;
              jpeg_decode_gpu(blobs, infos, dev, per_thread_hip_stream(),
                              frames);
              auto t3 = now();
              for (auto& f : frames) delete_buffer(dev, f.buffer);
              std::vector<MjpegSeg> segs;
              std::vector<u32> status;
              double ms = 0;
              mjpeg_index_gpu(base, s.size(), offsets, sizes,
                              base + offsets[0], ref->params, segs, status,
                              &ms, 1);
              if (it >= warmup) {
                t_index.push_back(secs(t0, t1));
                t_host.push_back(secs(t2, t3));
                t_kernel.push_back(ms * 1e-3);
              }
            }
          } catch (...) {
            delete_buffer(dev, d);
            throw;
          }
          delete_buffer(dev, d);
          py::dict out;
          out["index"] = t_index;
          out["host"] = t_host;
          out["index_kernel"] = t_kernel;
          return out;
        },
        py::arg("stream"), py::arg("offsets"), py::arg("sizes"), py::arg("h"),
        py::arg("w"), py::arg("c"), py::arg("windows") = 10,
        py::arg("warmup") = 3);
  // mjpeg_decode_gpu on samples laid out in `stream` (an item's bytes):
  // frames `want`, decoded from a device copy of the stream. Returns
  // (frames [n,H,W,C] u8, index_frames, fallback_frames).
  m.def("mjpeg_gpu_decode",
        [](py::bytes stream, std::vector<u64> offsets, std::vector<u64> sizes,
           std::vector<i64> want, i32 h, i32 w, i32 c) {
          SCA_CHECK(have_gpu(), "mjpeg_gpu_decode needs a GPU");
          std::string s = stream;
          SCA_CHECK(!offsets.empty() && offsets.size() == sizes.size(),
                    "one size per offset, at least one sample");
          VideoMetadata vm;
          vm.codec = "mjpeg";
          vm.height = h;
          vm.width = w;
          vm.channels = c;
          vm.num_frames = (i64)offsets.size();
          vm.sample_offsets = offsets;
          vm.sample_sizes = sizes;
          for (size_t i = 0; i < offsets.size(); ++i) {
            SCA_CHECK(offsets[i] <= s.size() &&
                          sizes[i] <= s.size() - offsets[i],
                      "sample " + std::to_string(i) +
                          " lies outside the stream");
            vm.keyframe_indices.push_back((i64)i);
          }
          std::shared_ptr<const MjpegRefHeader> ref;
          try {
            ref = mjpeg_ref_header((const u8*)s.data() + offsets[0], sizes[0]);
          } catch (const ScannerError&) {
            ref = std::make_shared<MjpegRefHeader>();
          }
          DeviceHandle dev{DeviceType::GPU, 0};
          MjpegGpuStats st;
          auto elems = mjpeg_decode_gpu((const u8*)s.data(), s.size(), vm, want,
                                        dev, *ref, 0, &st);
          size_t fsize = (size_t)h * w * c;
          py::array_t<u8> out({(i64)elems.size(), (i64)h, (i64)w, (i64)c});
          for (size_t i = 0; i < elems.size(); ++i) {
            memcpy_buffer(out.mutable_data() + i * fsize, CPU_DEVICE,
                          elems[i].buffer, dev, fsize);
            delete_buffer(dev, elems[i].buffer);
          }
          return py::make_tuple(out, st.index_frames, st.fallback_frames);
        },
        py::arg("stream"), py::arg("offsets"), py::arg("sizes"),
        py::arg("want"), py::arg("h"), py::arg("w"), py::arg("c"));

  // One item of a video column as stored: (bytes, video metadata).
  m.def("read_video_item",
        [](std::shared_ptr<Database> db, const std::string& table,
           const std::string& column, i32 item) {
          TableMetadata t = db->get_table(table);
          VideoMetadata vm = read_video_metadata(*db, t, column, item);
          auto bytes = db->storage()->read_all(
              db->paths().item(t.id, t.column_id(column), item));
          py::dict d;
          d["codec"] = vm.codec;
          d["height"] = vm.height;
          d["width"] = vm.width;
          d["channels"] = vm.channels;
          d["frame_type"] = (i32)vm.frame_type;
          d["num_frames"] = vm.num_frames;
          d["keyframe_indices"] = vm.keyframe_indices;
          d["sample_offsets"] = vm.sample_offsets;
          d["sample_sizes"] = vm.sample_sizes;
          return py::make_tuple(
              py::bytes((const char*)bytes.data(), bytes.size()), d);
        });

  m.def("read_column",
        [](std::shared_ptr<Database> db, const std::string& table,
           const std::string& column, std::vector<i64> rows) {
          TableMetadata t = db->get_table(table);
          if (rows.empty()) {
            for (i64 r = 0; r < t.num_rows(); ++r) rows.push_back(r);
          }
          py::list out;
          if (t.column_type(column) == ColumnType::Video) {
            auto items = items_for_rows(t, rows);
            size_t ri = 0;
            for (auto& ir : items) {
              VideoMetadata vm = read_video_metadata(*db, t, column, ir.item);
              std::vector<i64> local_rows;
              while (ri < rows.size() && rows[ri] < ir.row_end) {
                local_rows.push_back(rows[ri]);
                ++ri;
              }
              if (vm.codec == "raw") {
                ElementVector elems =
                    read_column_rows(*db, t, column, local_rows, 8);
                for (auto& e : elems) {
                  py::tuple shape =
                      py::make_tuple(vm.height, vm.width, vm.channels);
                  out.append(py::make_tuple(
                      py::bytes((const char*)e.buffer, e.size), shape,
                      (i32)vm.frame_type));
                  delete_buffer(CPU_DEVICE, e.buffer);
                }
              } else {
                // decode requested frames on CPU
                std::vector<i64> want;
                for (i64 r : local_rows) want.push_back(r - ir.row_start);
                auto stream = db->storage()->read_all(
                    db->paths().item(t.id, t.column_id(column), ir.item));
                std::vector<std::vector<u8>> frames;
                if (vm.codec == "mjpeg")
                  mjpeg_decode_cpu(stream.data(), stream.size(), vm, want,
                                   frames);
                else
                  svc_decode_cpu(stream.data(), stream.size(), vm, want,
                                 frames);
                for (auto& fb : frames) {
                  py::tuple shape =
                      py::make_tuple(vm.height, vm.width, vm.channels);
                  out.append(py::make_tuple(
                      py::bytes((const char*)fb.data(), fb.size()), shape,
                      (i32)vm.frame_type));
                }
              }
            }
          } else {
            ElementVector elems = read_column_rows(*db, t, column, rows, 8);
            for (auto& e : elems) {
              if (e.size == 0) {
                out.append(py::none());
              } else {
                out.append(py::bytes((const char*)e.buffer, e.size));
              }
              if (e.buffer) delete_buffer(CPU_DEVICE, e.buffer);
            }
          }
          return out;
        });

  // ---- analysis (exposed for unit tests) ----

  m.def("analyze_job_py", [](const py::bytes& graph_b, const py::bytes& job_b,
                             const py::dict& table_rows) {
    JobGraph g = graph_from_bytes(graph_b);
    validate_graph(g);
    JobBinding job = JobBinding::from_msgpack(mp_from_pybytes(job_b));
    std::map<std::string, i64> rows_map;
    for (auto item : table_rows)
      rows_map[item.first.cast<std::string>()] = item.second.cast<i64>();
    auto ja = analyze_job(g, job, [&](const SourceArgsC& s) {
      return rows_map.at(s.table);
    });
    py::dict d;
    py::list doms;
    for (auto& dom : ja.domains) {
      py::dict dd;
      dd["num_rows"] = dom.num_rows;
      dd["slice_level"] = dom.slice_level;
      dd["group_starts"] = dom.group_starts;
      doms.append(dd);
    }
    d["domains"] = doms;
    d["output_rows"] = ja.output_rows;
    return d;
  });

  m.def("task_plan_py", [](const py::bytes& graph_b, const py::bytes& job_b,
                           const py::dict& table_rows, i64 start, i64 end) {
    JobGraph g = graph_from_bytes(graph_b);
    validate_graph(g);
    JobBinding job = JobBinding::from_msgpack(mp_from_pybytes(job_b));
    std::map<std::string, i64> rows_map;
    for (auto item : table_rows)
      rows_map[item.first.cast<std::string>()] = item.second.cast<i64>();
    auto ja = analyze_job(g, job, [&](const SourceArgsC& s) {
      return rows_map.at(s.table);
    });
    auto plan = derive_task_plan(g, ja, job, start, end);
    py::dict d;
    py::list ops;
    for (auto& otp : plan.ops) {
      py::dict od;
      od["required_rows"] = otp.required_rows;
      od["compute_rows"] = otp.compute_rows;
      od["windows"] = otp.windows;
      od["remap"] = otp.remap;
      py::list rb;
      for (u8 v : otp.reset_before) rb.append((bool)v);
      od["reset_before"] = rb;
      ops.append(od);
    }
    d["ops"] = ops;
    py::dict lr;
    for (auto& kv : plan.load_rows) lr[py::int_(kv.first)] = kv.second;
    d["load_rows"] = lr;
    return d;
  });

  // ---- execution ----

  py::class_<PreparedTask, std::shared_ptr<PreparedTask>>(m, "PreparedTask");

  py::class_<LocalExecutor>(m, "LocalExecutor")
      .def(py::init([](std::shared_ptr<Database> db, const py::bytes& graph_b,
                       const py::bytes& jobs_b, const py::dict& perf,
                       std::vector<i32> gpu_ids) {
             return new LocalExecutor(db, graph_from_bytes(graph_b),
                                      jobs_from_bytes(jobs_b),
                                      perf_from_dict(perf), gpu_ids);
           }),
           py::arg("db"), py::arg("graph"), py::arg("jobs"), py::arg("perf"),
           py::arg("gpu_ids") = std::vector<i32>{})
      .def("run",
           [](LocalExecutor& ex) {
             py::gil_scoped_release rel;
             ex.run();
           })
      .def("prepare", &LocalExecutor::prepare,
           py::arg("create_outputs") = true)
      .def("all_tasks",
           [](LocalExecutor& ex) {
             py::list out;
             for (auto& t : ex.all_tasks())
               out.append(py::make_tuple(t.job, t.task, t.start, t.end));
             return out;
           })
      .def("process_task",
           [](LocalExecutor& ex, i32 instance, i32 job, i32 task, i64 start,
              i64 end) {
             TaskDesc t{job, task, start, end};
             py::gil_scoped_release rel;
             ex.process_task_public(instance, t);
           })
      .def("prepare_task",
           [](LocalExecutor& ex, i32 job, i32 task, i64 start, i64 end) {
             TaskDesc t{job, task, start, end};
             py::gil_scoped_release rel;
             return ex.prepare_task_public(t);
           })
      .def("process_prepared",
           [](LocalExecutor& ex, i32 instance,
              std::shared_ptr<PreparedTask> pt) {
             py::gil_scoped_release rel;
             ex.process_prepared_public(instance, pt);
           })
      .def("finalize_job", &LocalExecutor::finalize_job)
      .def("tasks_done", &LocalExecutor::tasks_done)
      .def("total_output_rows", &LocalExecutor::total_output_rows)
      .def("profilers",
           [](LocalExecutor& ex) { return profilers_to_py(ex.profilers()); });
}
