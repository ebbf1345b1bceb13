// tests/cxx/mc_driver.cpp -- drives the C++ layers of the surface reconstruction: the mesh PLY reader and writer of mvr/io.hpp,
// pcl::MarchingCubesHoppe / pcl::PolygonMesh / pcl::Vertices in mvr/registration.hpp, ScanCloud::reconstructMesh and
// Registrator::saveRegisteredMesh in mvr/registrator.hpp.  tests/test_mc_host.py (the first mode, no GPU) and
// tests/test_gpu_mc_cxx.py compile it and compare what it writes with the Python path.
//
// usage: mc_driver roundtrip <in.ply> <out.ply>      loadPLYFile(mesh) -> savePLYFile; prints "<vertices> <faces>"; exit 4: not read
//        mc_driver shim <cloud.bin> <res> <extend> <weld> <folder>
//                   (cloud.bin: n x 6 floats, x y z nx ny nz) pcl::MarchingCubesHoppe in PCL's order of calls -> <folder>/mesh.ply,
//                   <folder>/scan.ply (ScanCloud::reconstructMesh); prints JSON
//        mc_driver registered <views> <points> <config_id> <res> <folder>
//                   three synthetic views on a platter, platter removal on -> <folder>/mesh.ply, <folder>/points.pcd,
//                   <folder>/merged.bin (the merged cloud the mesh was made from, n x 6 floats); prints JSON
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define MVR_ALIAS_PCL
#include "mvr/registrator.hpp"

using namespace mvr;

static bool write_floats(const std::string &path, const std::vector<float> &v)
{
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
  std::fclose(f);
  return ok;
}

int main(int argc, char **argv)
{
  if (argc < 2) { std::fprintf(stderr, "usage: %s roundtrip|shim|registered ...\n", argv[0]); return 2; }
  const std::string mode = argv[1];
  try {
    if (mode == "roundtrip" && argc == 4) {
      pcl::PolygonMesh mesh;
      mesh.cloud.push_back(pcl::PointXYZ(9.f, 9.f, 9.f));      // a failed read leaves the mesh as it was
      if (!pcl::io::loadPLYFile(argv[2], mesh)) return mesh.cloud.size() == 1 && mesh.polygons.empty() ? 4 : 5;
      if (!pcl::io::savePLYFile(argv[3], mesh)) return 6;
      std::printf("%zu %zu\n", mesh.cloud.size(), mesh.polygons.size());
      return 0;
    }
    if (mode == "shim" && argc == 7) {
      const int res = std::atoi(argv[3]);
      const float extend = (float)std::atof(argv[4]);
      const bool weld = std::atoi(argv[5]) != 0;
      const std::string folder = argv[6];
      FILE *f = std::fopen(argv[2], "rb");
      if (!f) return 3;
      std::vector<float> raw;
      float rec[6];
      while (std::fread(rec, sizeof(float), 6, f) == 6) raw.insert(raw.end(), rec, rec + 6);
      std::fclose(f);
      const size_t n = raw.size() / 6;
      pcl::PointCloud<pcl::PointNormal>::Ptr cloud(new pcl::PointCloud<pcl::PointNormal>);
      cloud->resize(n);
      for (size_t i = 0; i < n; ++i) {
        pcl::PointNormal &q = cloud->points[i];
        q.x = raw[6 * i]; q.y = raw[6 * i + 1]; q.z = raw[6 * i + 2];
        q.normal_x = raw[6 * i + 3]; q.normal_y = raw[6 * i + 4]; q.normal_z = raw[6 * i + 5];
      }
      // PCL's tutorial order of calls
      pcl::search::KdTree<pcl::PointNormal>::Ptr tree(new pcl::search::KdTree<pcl::PointNormal>);
      pcl::MarchingCubesHoppe<pcl::PointNormal> mc;
      int rx = 0, ry = 0, rz = 0;
      mc.getGridResolution(rx, ry, rz);
      std::printf("{\"defaults\": [%d, %d, %d, %g, %g, %g, %d], ", rx, ry, rz, mc.getIsoLevel(), mc.getPercentageExtendGrid(), mc.getDistanceIgnore(),
                  (int)mc.getWeld());
      pcl::PolygonMesh mesh;
      mc.reconstruct(mesh);                                      // no input: an error is printed, the mesh stays empty
      std::printf("\"no_input\": [%zu, %zu], ", mesh.cloud.size(), mesh.polygons.size());
      mc.setInputCloud(cloud);
      mc.setSearchMethod(tree);
      mc.setGridResolution(res, res, res);
      mc.setIsoLevel(0.f);
      mc.setPercentageExtendGrid(extend);
      mc.setDistanceIgnore(-1.f);
      mc.setWeld(weld);
      mc.reconstruct(mesh);
      mc.getGridResolution(rx, ry, rz);
      if (!pcl::io::savePLYFile(folder + "/mesh.ply", mesh)) return 6;
      pcl::PolygonMesh back;
      if (!pcl::io::loadPLYFile(folder + "/mesh.ply", back)) return 7;
      bool same = back.cloud.size() == mesh.cloud.size() && back.polygons.size() == mesh.polygons.size();
      for (size_t i = 0; same && i < mesh.cloud.size(); ++i) same = std::memcmp(back.cloud.points[i].data, mesh.cloud.points[i].data, 12) == 0;
      for (size_t t = 0; same && t < mesh.polygons.size(); ++t) same = back.polygons[t].vertices == mesh.polygons[t].vertices;
      // the two-argument overload: the same triangles, vertices as PointNormal with zero normals
      pcl::PointCloud<pcl::PointNormal> pts;
      std::vector<pcl::Vertices> polys;
      mc.reconstruct(pts, polys);
      bool overload = pts.size() == mesh.cloud.size() && polys.size() == mesh.polygons.size();
      for (size_t i = 0; overload && i < pts.size(); ++i)
        overload = std::memcmp(pts.points[i].data, mesh.cloud.points[i].data, 12) == 0 && pts.points[i].normal_x == 0.f && pts.points[i].normal_z == 0.f;
      mc.setGridResolution(1, res, res);                         // refused (rule M12): printed, empty
      pcl::PolygonMesh none;
      mc.reconstruct(none);
      // the driver's member on a scan that holds the same points and normals
      ScanCloud scan;
      scan.points.resize(n);
      scan.rich.resize(n);
      for (size_t i = 0; i < n; ++i) {
        scan.points.points[i] = pcl::PointXYZ(raw[6 * i], raw[6 * i + 1], raw[6 * i + 2]);
        io::RichPoint &q = scan.rich[i];
        q.x = raw[6 * i]; q.y = raw[6 * i + 1]; q.z = raw[6 * i + 2];
        q.normal_x = raw[6 * i + 3]; q.normal_y = raw[6 * i + 4]; q.normal_z = raw[6 * i + 5];
      }
      ScanCloud::MeshParams mp;
      mp.res[0] = mp.res[1] = mp.res[2] = res;
      mp.percentage_extend_grid = extend;
      mp.weld = weld;
      pcl::PolygonMesh sm, by_voxel, too_fine, bare_mesh;
      const bool scan_ok = scan.reconstructMesh(mp, sm) && pcl::io::savePLYFile(folder + "/scan.ply", sm);
      mp.voxel_size = 10.0;                                      // res = ceil(extent / 10) + 1 per axis
      const bool voxel_ok = scan.reconstructMesh(mp, by_voxel);
      mp.voxel_size = 1.0e-4;                                    // a lattice far above 2^27 vertices: refused
      const bool fine_ok = scan.reconstructMesh(mp, too_fine);
      ScanCloud bare;
      bare.points = scan.points;                                 // no rich records: no normals
      mp.voxel_size = 0.0;
      const bool bare_ok = bare.reconstructMesh(mp, bare_mesh);
      std::printf("\"res\": [%d, %d, %d], \"mesh\": [%zu, %zu], \"read_back\": %d, \"overload\": %d, \"refused\": [%zu, %zu], \"scan\": [%d, %zu, %zu], "
                  "\"by_voxel\": [%d, %zu], \"too_fine\": [%d, %zu], \"bare\": [%d, %zu]}\n",
                  rx, ry, rz, mesh.cloud.size(), mesh.polygons.size(), (int)same, (int)overload, none.cloud.size(), none.polygons.size(), (int)scan_ok,
                  sm.cloud.size(), sm.polygons.size(), (int)voxel_ok, by_voxel.polygons.size(), (int)fine_ok, too_fine.polygons.size(), (int)bare_ok,
                  bare_mesh.polygons.size());
      return 0;
    }
    if (mode == "registered" && argc == 7) {
      const int V = std::atoi(argv[2]);
      const size_t N = (size_t)std::atol(argv[3]);
      const int config = std::atoi(argv[4]), res = std::atoi(argv[5]);
      const std::string folder = argv[6];
      mvr_synth_params sp;
      mvr_synth_default(&sp, 12, config);
      // the platter: a disc of points 115 mm along the axis from the pivot, its normals along the axis -- the same points in every
      // view, since a turn about the axis maps the disc to itself
      double ax[3] = {sp.axis[0], sp.axis[1], sp.axis[2]};
      const double an = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
      for (double &a : ax) a /= an;
      double u[3] = {ax[1], -ax[0], 0.0};
      const double un = std::sqrt(u[0] * u[0] + u[1] * u[1]);
      for (double &a : u) a /= un;
      const double w[3] = {ax[1] * u[2] - ax[2] * u[1], ax[2] * u[0] - ax[0] * u[2], ax[0] * u[1] - ax[1] * u[0]};
      const size_t P = N / 4;
      TurntableModel model;
      model.views.resize(V);
      for (int v = 0; v < V; ++v) {
        ScanCloud &pc = model.views[v];
        pc.view = v;
        pc.points.resize(N);
        std::vector<float> nrm(4 * N);
        if (mvr_synth_view(&sp, v, N, pc.points.points[0].data, nrm.data()) != MVR_OK) return 3;
        for (size_t i = 0; i < P; ++i) {
          const double r = 110.0 * std::sqrt((double)(i + 1) / (double)P), a = 2.399963229728653 * (double)i + 0.37 * v;
          const double c = r * std::cos(a), s = r * std::sin(a);
          pc.points.push_back(pcl::PointXYZ((float)(sp.pivot[0] + 115.0 * ax[0] + c * u[0] + s * w[0]), (float)(sp.pivot[1] + 115.0 * ax[1] + c * u[1] + s * w[1]),
                                            (float)(sp.pivot[2] + 115.0 * ax[2] + c * u[2] + s * w[2])));
          for (int k = 0; k < 3; ++k) nrm.push_back((float)-ax[k]);
          nrm.push_back(0.f);
        }
        pc.rich.resize(pc.points.size());
        for (size_t i = 0; i < pc.points.size(); ++i) {
          io::RichPoint &q = pc.rich[i];
          q.x = pc.points.points[i].x; q.y = pc.points.points[i].y; q.z = pc.points.points[i].z;
          q.normal_x = nrm[4 * i]; q.normal_y = nrm[4 * i + 1]; q.normal_z = nrm[4 * i + 2];
        }
      }
      Registrator reg(&model);
      reg.setPivotPoint(sp.pivot[0], sp.pivot[1], sp.pivot[2]);
      reg.setAxisNormal(sp.axis[0], sp.axis[1], sp.axis[2]);
      for (int v = 0; v < V; ++v) { model.views[v].initRotation(reg); model.views[v].setRegisterState(true); }
      ScanCloud::MeshParams mp;
      mp.res[0] = mp.res[1] = mp.res[2] = res;
      mp.percentage_extend_grid = 0.1f;
      pcl::PolygonMesh off_mesh, mesh;
      const size_t t_off = reg.saveRegisteredMesh(0, folder + "/off", mp, &off_mesh);      // the platter still in
      reg.setPlatterRemoval(1.0, 0.1, 1000, 7);
      io::RichCloud merged;
      const size_t n_points = reg.saveRegisteredPoints(0, folder, &merged), taken = reg.lastPlatterPoints();
      const size_t t_on = reg.saveRegisteredMesh(0, folder, mp, &mesh), taken_mesh = reg.lastPlatterPoints();
      std::vector<float> flat;
      for (const io::RichPoint &q : merged) { const float r6[6] = {q.x, q.y, q.z, q.normal_x, q.normal_y, q.normal_z}; flat.insert(flat.end(), r6, r6 + 6); }
      if (!write_floats(folder + "/merged.bin", flat)) return 6;
      // a registered view without rich records: the merge has no normals -- nothing written, 0
      model.views[1].rich.clear();
      const size_t t_bare = reg.saveRegisteredMesh(0, folder + "/bare", mp);
      std::printf("{\"platter_points\": %zu, \"off\": [%zu, %zu], \"on\": [%zu, %zu, %zu], \"points\": [%zu, %zu, %zu], \"bare\": %zu}\n", (size_t)V * P, t_off,
                  off_mesh.polygons.size(), t_on, mesh.cloud.size(), mesh.polygons.size(), n_points, taken, taken_mesh, t_bare);
      return 0;
    }
    std::fprintf(stderr, "mc_driver: bad arguments\n");
    return 2;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "mc_driver: %s\n", e.what());
    return 1;
  }
}
