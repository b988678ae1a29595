// Mitsuba 0.5/0.6 XML scene loading for the `path` hot path: the XML parser,
// the mesh file readers and the SceneHandler that turns a document into
// SceneBuilder calls (builder.cpp holds the plugin constructors).
//
// Mirrors the SceneHandler semantics the configs need
// (reference src/librender/scenehandler.cpp:70-106 tag table, :461-625
// value tags, :700-780 object creation) and the shape/BSDF/emitter plugin
// constructors' parameter parsing:
//   shapes  ply (src/shapes/ply.cpp), obj (src/shapes/obj.cpp),
//           rectangle (src/shapes/rectangle.cpp), cube (src/shapes/cube.cpp),
//           shapegroup/instance (src/shapes/shapegroup.cpp, instance.cpp;
//           flattened into world-space meshes here)
//   bsdfs   diffuse (diffuse.cpp:75-84), roughconductor
//           (roughconductor.cpp:168-203, microfacet.h:99-146),
//           dielectric (dielectric.cpp:148-170)
//   emitter area (area.cpp:67-78)
//   sensor  perspective, thinlens (perspective.cpp, thinlens.cpp:122-143, sensor.cpp:150-278)
//   film    hdrfilm (hdrfilm.cpp:209-220), rfilter gaussian/box
//   sampler independent (independent.cpp:55-58), halton (halton.cpp:113-121),
//           hammersley (hammersley.cpp:93-101), ldsampler (ldsampler.cpp:82-95)
//   integrator path (integrator.cpp:199-234)
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <sstream>

#include <zlib.h>

#include "scene.h"

namespace mtsh {

static std::runtime_error err(const std::string &m) { return std::runtime_error(m); }

// ---------------------------------------------------------------------------
// Minimal XML DOM
// ---------------------------------------------------------------------------
struct XNode {
    std::string tag;
    std::vector<std::pair<std::string, std::string>> attrs;
    std::vector<std::unique_ptr<XNode>> children;
    int line = 0;
    bool hasAttr(const std::string &k) const {
        for (auto &a : attrs) if (a.first == k) return true;
        return false;
    }
    std::string attr(const std::string &k, const std::string &def = "") const {
        for (auto &a : attrs) if (a.first == k) return a.second;
        return def;
    }
};

namespace {
struct XParser {
    const std::string &s;
    size_t i = 0;
    int line = 1;
    std::string file;
    explicit XParser(const std::string &src, const std::string &f) : s(src), file(f) {}
    [[noreturn]] void fail(const std::string &m) {
        throw err(file + ":" + std::to_string(line) + ": XML parse error: " + m);
    }
    void adv(size_t n = 1) {
        for (size_t k = 0; k < n && i < s.size(); ++k, ++i)
            if (s[i] == '\n') ++line;
    }
    bool starts(const char *p) const { return s.compare(i, strlen(p), p) == 0; }
    void ws() { while (i < s.size() && isspace((unsigned char)s[i])) adv(); }
    void skipMisc() {
        for (;;) {
            ws();
            if (starts("<!--")) {
                size_t e = s.find("-->", i);
                if (e == std::string::npos) fail("unterminated comment");
                adv(e + 3 - i);
            } else if (starts("<?")) {
                size_t e = s.find("?>", i);
                if (e == std::string::npos) fail("unterminated declaration");
                adv(e + 2 - i);
            } else if (starts("<!")) {
                size_t e = s.find('>', i);
                if (e == std::string::npos) fail("unterminated doctype");
                adv(e + 1 - i);
            } else {
                return;
            }
        }
    }
    static std::string unescape(const std::string &v) {
        std::string o;
        for (size_t k = 0; k < v.size(); ++k) {
            if (v[k] == '&') {
                size_t e = v.find(';', k);
                std::string ent = v.substr(k + 1, e - k - 1);
                if (ent == "lt") o += '<';
                else if (ent == "gt") o += '>';
                else if (ent == "amp") o += '&';
                else if (ent == "quot") o += '"';
                else if (ent == "apos") o += '\'';
                else o += "&" + ent + ";";
                k = e;
            } else {
                o += v[k];
            }
        }
        return o;
    }
    std::string name() {
        size_t b = i;
        while (i < s.size() && (isalnum((unsigned char)s[i]) || s[i] == '_' || s[i] == '-' || s[i] == ':' || s[i] == '.')) adv();
        if (b == i) fail("expected a name");
        return s.substr(b, i - b);
    }
    std::unique_ptr<XNode> element() {
        skipMisc();
        if (i >= s.size() || s[i] != '<') fail("expected '<'");
        adv();
        auto node = std::make_unique<XNode>();
        node->line = line;
        node->tag = name();
        for (;;) {
            ws();
            if (starts("/>")) { adv(2); return node; }
            if (starts(">")) { adv(); break; }
            std::string k = name();
            ws();
            if (i >= s.size() || s[i] != '=') fail("expected '=' after attribute " + k);
            adv(); ws();
            char q = s[i];
            if (q != '"' && q != '\'') fail("expected quoted attribute value");
            adv();
            size_t e = s.find(q, i);
            if (e == std::string::npos) fail("unterminated attribute value");
            std::string v = unescape(s.substr(i, e - i));
            adv(e + 1 - i);
            node->attrs.emplace_back(k, v);
        }
        for (;;) {
            // skip text content
            while (i < s.size() && s[i] != '<') adv();
            if (starts("<!--")) { skipMisc(); continue; }
            if (starts("</")) {
                adv(2);
                std::string n = name();
                if (n != node->tag) fail("mismatched </" + n + "> for <" + node->tag + ">");
                ws();
                if (s[i] != '>') fail("expected '>'");
                adv();
                return node;
            }
            if (i >= s.size()) fail("unexpected end of file inside <" + node->tag + ">");
            node->children.push_back(element());
        }
    }
};

std::string readFile(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw err("Unable to open \"" + path + "\"");
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

std::string dirName(const std::string &p) {
    size_t k = p.find_last_of('/');
    return k == std::string::npos ? std::string(".") : p.substr(0, k);
}

std::string lower(std::string s) {
    for (auto &c : s) c = (char)tolower((unsigned char)c);
    return s;
}

std::vector<std::string> tokenize(const std::string &s, const char *delims) {
    std::vector<std::string> out;
    std::string cur;
    for (char c : s) {
        if (strchr(delims, c)) {
            if (!cur.empty()) out.push_back(cur);
            cur.clear();
        } else {
            cur += c;
        }
    }
    if (!cur.empty()) out.push_back(cur);
    return out;
}

float parseF(const std::string &v, int line) {
    char *end = nullptr;
    std::string t = v;
    while (!t.empty() && isspace((unsigned char)t.back())) t.pop_back();
    size_t b = 0;
    while (b < t.size() && isspace((unsigned char)t[b])) ++b;
    t = t.substr(b);
    float f = strtof(t.c_str(), &end);
    if (t.empty() || *end != '\0') throw err("line " + std::to_string(line) + ": could not parse floating point value \"" + v + "\"");
    return f;
}
}  // namespace

// ---------------------------------------------------------------------------
// Mesh loaders
// ---------------------------------------------------------------------------
namespace {
struct PlyProp {
    std::string name, type, countType;
    bool list = false;
};
struct PlyElem {
    std::string name;
    size_t count = 0;
    std::vector<PlyProp> props;
};
size_t plyTypeSize(const std::string &t) {
    if (t == "char" || t == "uchar" || t == "int8" || t == "uint8") return 1;
    if (t == "short" || t == "ushort" || t == "int16" || t == "uint16") return 2;
    if (t == "int" || t == "uint" || t == "float" || t == "int32" || t == "uint32" || t == "float32") return 4;
    if (t == "double" || t == "float64") return 8;
    throw err("PLY: unknown property type " + t);
}
double plyRead(const unsigned char *p, const std::string &t, bool swap) {
    unsigned char b[8];
    size_t n = plyTypeSize(t);
    for (size_t k = 0; k < n; ++k) b[k] = swap ? p[n - 1 - k] : p[k];
    if (t == "char" || t == "int8") return (double)(int8_t)b[0];
    if (t == "uchar" || t == "uint8") return (double)b[0];
    if (t == "short" || t == "int16") { int16_t v; memcpy(&v, b, 2); return v; }
    if (t == "ushort" || t == "uint16") { uint16_t v; memcpy(&v, b, 2); return v; }
    if (t == "int" || t == "int32") { int32_t v; memcpy(&v, b, 4); return v; }
    if (t == "uint" || t == "uint32") { uint32_t v; memcpy(&v, b, 4); return v; }
    if (t == "float" || t == "float32") { float v; memcpy(&v, b, 4); return v; }
    double v; memcpy(&v, b, 8); return v;
}
}  // namespace

void loadPLY(const std::string &path, Mesh &mesh) {
    std::string data = readFile(path);
    size_t hdrEnd = data.find("end_header");
    if (data.compare(0, 3, "ply") != 0 || hdrEnd == std::string::npos)
        throw err("\"" + path + "\": not a PLY file");
    size_t bodyStart = data.find('\n', hdrEnd);
    if (bodyStart == std::string::npos) throw err("PLY: truncated header");
    ++bodyStart;
    std::istringstream hs(data.substr(0, hdrEnd));
    std::string line, format;
    std::vector<PlyElem> elems;
    while (std::getline(hs, line)) {
        auto tok = tokenize(line, " \t\r");
        if (tok.empty()) continue;
        if (tok[0] == "format") format = tok.at(1);
        else if (tok[0] == "element") { PlyElem e; e.name = tok.at(1); e.count = std::stoull(tok.at(2)); elems.push_back(e); }
        else if (tok[0] == "property") {
            if (elems.empty()) throw err("PLY: property before element");
            PlyProp p;
            if (tok.at(1) == "list") { p.list = true; p.countType = tok.at(2); p.type = tok.at(3); p.name = tok.at(4); }
            else { p.type = tok.at(1); p.name = tok.at(2); }
            elems.back().props.push_back(p);
        }
    }
    bool ascii = format == "ascii";
    bool swap = format == "binary_big_endian";
    if (!ascii && format != "binary_little_endian" && !swap) throw err("PLY: unknown format " + format);

    const unsigned char *p = (const unsigned char *)data.data() + bodyStart;
    const unsigned char *end = (const unsigned char *)data.data() + data.size();
    std::istringstream as(ascii ? data.substr(bodyStart) : std::string());

    bool hasN = false, hasUV = false;
    for (auto &e : elems) {
        if (e.name != "vertex") continue;
        for (auto &pr : e.props) {
            if (pr.name == "nx") hasN = true;
            if (pr.name == "u" || pr.name == "s" || pr.name == "texture_u" || pr.name == "texture_s") hasUV = true;
        }
    }
    auto readVal = [&](const std::string &t) -> double {
        if (ascii) { double v; if (!(as >> v)) throw err("PLY: truncated ascii body"); return v; }
        size_t n = plyTypeSize(t);
        if (p + n > end) throw err("PLY: truncated binary body");
        double v = plyRead(p, t, swap);
        p += n;
        return v;
    };
    for (auto &e : elems) {
        if (e.name == "vertex") {
            mesh.p.resize(e.count);
            if (hasN) mesh.n.resize(e.count);
            if (hasUV) mesh.uv.resize(2 * e.count);
            for (size_t v = 0; v < e.count; ++v) {
                for (auto &pr : e.props) {
                    if (pr.list) { size_t c = (size_t)readVal(pr.countType); for (size_t k = 0; k < c; ++k) readVal(pr.type); continue; }
                    double x = readVal(pr.type);
                    const std::string &nm = pr.name;
                    if (nm == "x") mesh.p[v].x = (float)x;
                    else if (nm == "y") mesh.p[v].y = (float)x;
                    else if (nm == "z") mesh.p[v].z = (float)x;
                    else if (nm == "nx") mesh.n[v].x = (float)x;
                    else if (nm == "ny") mesh.n[v].y = (float)x;
                    else if (nm == "nz") mesh.n[v].z = (float)x;
                    else if (nm == "u" || nm == "s" || nm == "texture_u" || nm == "texture_s") mesh.uv[2 * v] = (float)x;
                    else if (nm == "v" || nm == "t" || nm == "texture_v" || nm == "texture_t") mesh.uv[2 * v + 1] = (float)x;
                }
            }
        } else if (e.name == "face") {
            mesh.idx.reserve(e.count * 3);
            for (size_t f = 0; f < e.count; ++f) {
                for (auto &pr : e.props) {
                    if (!pr.list) { readVal(pr.type); continue; }
                    size_t c = (size_t)readVal(pr.countType);
                    uint32_t ids[4];
                    if (pr.name != "vertex_indices" && pr.name != "vertex_index") { for (size_t k = 0; k < c; ++k) readVal(pr.type); continue; }
                    if (c != 3 && c != 4) throw err("Encountered a face with " + std::to_string(c) + " vertices! Only triangle and quad-based PLY meshes are supported for now.");
                    for (size_t k = 0; k < c; ++k) {
                        double id = readVal(pr.type);
                        if (id < 0 || (size_t)id >= mesh.p.size()) throw err("PLY: vertex index out of range");
                        ids[k] = (uint32_t)id;
                    }
                    // ply.cpp:276-289 (quad -> (0,1,2), (3,0,2))
                    mesh.idx.insert(mesh.idx.end(), {ids[0], ids[1], ids[2]});
                    if (c == 4) mesh.idx.insert(mesh.idx.end(), {ids[3], ids[0], ids[2]});
                }
            }
        } else {
            for (size_t r = 0; r < e.count; ++r)
                for (auto &pr : e.props) {
                    if (pr.list) { size_t c = (size_t)readVal(pr.countType); for (size_t k = 0; k < c; ++k) readVal(pr.type); }
                    else readVal(pr.type);
                }
        }
    }
}

void loadOBJ(const std::string &path, Mesh &mesh, bool flipTexCoords, bool collapse) {
    // Simplified obj.cpp: all groups collapsed into one mesh, polygon fans
    // (obj.cpp:309-322), vertices deduplicated by (p, n, uv) (obj.cpp:577-660).
    // The reference flushes one TriMesh per `g` / `usemtl` that follows faces
    // (obj.cpp:258-295, unless `collapse`): those boundaries are kept in
    // mesh.elemStart for the shapeIndex / primIndex fields
    std::ifstream f(path);
    if (!f) throw err("Unable to open \"" + path + "\"");
    std::vector<V3> P, N;
    std::vector<std::pair<float, float>> T;
    struct Key { int p, n, t; bool operator<(const Key &o) const { return std::tie(p, n, t) < std::tie(o.p, o.n, o.t); } };
    std::map<Key, uint32_t> vmap;
    std::vector<Key> verts;
    std::vector<uint32_t> idx;
    bool anyN = false, anyT = false;
    std::string line;
    auto parseIdx = [&](const std::string &tok) {
        Key k{0, 0, 0};
        auto parts = std::vector<std::string>();
        std::string cur;
        for (char c : tok) { if (c == '/') { parts.push_back(cur); cur.clear(); } else cur += c; }
        parts.push_back(cur);
        auto conv = [](const std::string &s, size_t n) -> int {
            if (s.empty()) return 0;
            int v = std::stoi(s);
            return v < 0 ? (int)n + v + 1 : v;
        };
        k.p = conv(parts[0], P.size());
        if (parts.size() > 1) k.t = conv(parts[1], T.size());
        if (parts.size() > 2) k.n = conv(parts[2], N.size());
        if (k.n) anyN = true;
        if (k.t) anyT = true;
        auto it = vmap.find(k);
        if (it != vmap.end()) return it->second;
        uint32_t id = (uint32_t)verts.size();
        vmap[k] = id;
        verts.push_back(k);
        return id;
    };
    std::vector<uint32_t> elemStart{0u};
    while (std::getline(f, line)) {
        std::istringstream iss(line);
        std::string t;
        if (!(iss >> t)) continue;
        if ((t == "g" || t == "usemtl") && !collapse) {
            const uint32_t nTri = (uint32_t)(idx.size() / 3);
            if (nTri > elemStart.back()) elemStart.push_back(nTri);
            continue;
        }
        if (t == "v") { V3 v; iss >> v.x >> v.y >> v.z; P.push_back(v); }
        else if (t == "vn") { V3 v; iss >> v.x >> v.y >> v.z; N.push_back(v); }
        else if (t == "vt") { float u = 0, v = 0; iss >> u >> v; if (flipTexCoords) v = 1 - v; T.emplace_back(u, v); }
        else if (t == "f") {
            std::vector<std::string> toks;
            std::string s;
            while (iss >> s) toks.push_back(s);
            if (toks.size() < 3) continue;
            uint32_t a = parseIdx(toks[0]), b = parseIdx(toks[1]), c = parseIdx(toks[2]);
            idx.insert(idx.end(), {a, b, c});
            for (size_t k = 3; k < toks.size(); ++k) {
                b = c;
                c = parseIdx(toks[k]);
                idx.insert(idx.end(), {a, b, c});
            }
        }
    }
    mesh.p.resize(verts.size());
    if (anyN) mesh.n.resize(verts.size());
    if (anyT) mesh.uv.resize(2 * verts.size());
    for (size_t i = 0; i < verts.size(); ++i) {
        const Key &k = verts[i];
        if (k.p <= 0 || (size_t)k.p > P.size()) throw err("OBJ: vertex index out of range");
        mesh.p[i] = P[k.p - 1];
        if (anyN) mesh.n[i] = (k.n > 0 && (size_t)k.n <= N.size()) ? N[k.n - 1] : V3(0.0f);
        if (anyT && k.t > 0 && (size_t)k.t <= T.size()) { mesh.uv[2 * i] = T[k.t - 1].first; mesh.uv[2 * i + 1] = T[k.t - 1].second; }
    }
    if (elemStart.size() > 1 && elemStart.back() == idx.size() / 3) elemStart.pop_back();   // a trailing group without faces
    if (elemStart.size() > 1) mesh.elemStart = elemStart;
    mesh.idx = std::move(idx);
}

// Mitsuba's `serialized` mesh container (src/shapes/serialized.cpp:64-145,
// TriMesh::loadCompressed / readHeader / readOffset in
// src/librender/trimesh.cpp:175-300): per mesh an uncompressed header
// (uint16 0x041C, uint16 version 3 or 4) followed by a zlib (DEFLATE) stream
// holding uint32 flags, [v4: a null-terminated name], uint64 vertex and
// triangle counts, positions, optional normals / texcoords / colors (float32,
// or float64 with flag 0x2000), and uint32 triangle indices.  The file ends
// with a dictionary of the meshes' start offsets (v4: uint64, v3: uint32) and
// a uint32 mesh count.  Vertex colors are read and dropped (no texture
// plugins in this build).
namespace {
enum { kSerHasNormals = 0x0001, kSerHasTexcoords = 0x0002, kSerHasColors = 0x0008, kSerDouble = 0x2000 };

class Inflater {
public:
    Inflater(const std::string &data, size_t offset, const std::string &path) : path_(path) {
        memset(&z_, 0, sizeof(z_));
        if (inflateInit(&z_) != Z_OK) throw err("\"" + path + "\": inflateInit failed");
        z_.next_in = (Bytef *)data.data() + offset;
        z_.avail_in = (uInt)(data.size() - offset);
    }
    ~Inflater() { inflateEnd(&z_); }
    void read(void *dst, size_t n) {
        z_.next_out = (Bytef *)dst;
        z_.avail_out = (uInt)n;
        while (z_.avail_out > 0) {
            int rc = inflate(&z_, Z_SYNC_FLUSH);
            if (rc == Z_STREAM_END && z_.avail_out > 0)
                throw err("\"" + path_ + "\": unexpected end of the compressed mesh stream");
            if (rc != Z_OK && rc != Z_STREAM_END)
                throw err("\"" + path_ + "\": corrupt compressed mesh stream (zlib error " + std::to_string(rc) + ")");
        }
    }
    template <class T> T get() { T v; read(&v, sizeof(T)); return v; }
    std::string cstring() {
        std::string s;
        for (char c; (c = get<char>()) != 0;) s += c;
        return s;
    }
    // readHelper (trimesh.cpp:150-172): single or double precision to float
    void floats(std::vector<float> &out, size_t n, bool dbl) {
        out.resize(n);
        if (!dbl) { read(out.data(), n * sizeof(float)); return; }
        std::vector<double> tmp(n);
        read(tmp.data(), n * sizeof(double));
        for (size_t i = 0; i < n; ++i) out[i] = (float)tmp[i];
    }
private:
    z_stream z_;
    std::string path_;
};

template <class T> T leAt(const std::string &d, size_t off) { T v; memcpy(&v, d.data() + off, sizeof(T)); return v; }
}  // namespace

void loadSerialized(const std::string &path, int shapeIndex, Mesh &mesh) {
    const std::string data = readFile(path);
    auto header = [&](size_t off) -> int {
        if (off + 4 > data.size()) throw err("\"" + path + "\": truncated file");
        const uint16_t format = leAt<uint16_t>(data, off), version = leAt<uint16_t>(data, off + 2);
        if (format == 0x1C04)
            throw err("Encountered a geometry file generated by an old version of Mitsuba. Please re-import the scene to update this file to the current format.");
        if (format != 0x041C) throw err("\"" + path + "\": Encountered an invalid file format!");
        if (version != 3 && version != 4) throw err("\"" + path + "\": Encountered an incompatible file version!");
        return version;
    };
    if (shapeIndex < 0) throw err("Shape index must be nonnegative!");
    const int version = header(0);
    size_t offset = 0;
    if (shapeIndex != 0) {
        // readOffset (trimesh.cpp:272-291); the dictionary sits at the end
        if (data.size() < 8) throw err("\"" + path + "\": truncated file");
        const uint32_t count = leAt<uint32_t>(data, data.size() - 4);
        if (shapeIndex >= (int)count)
            throw err("Unable to unserialize mesh, shape index is out of range! (requested " + std::to_string(shapeIndex) +
                      " out of 0.." + std::to_string((int)count - 1) + ")");
        if (version == 4) {
            const size_t at = data.size() - 8 * (size_t)(count - shapeIndex) - 4;
            if (at > data.size()) throw err("\"" + path + "\": corrupt offset dictionary");
            offset = (size_t)leAt<uint64_t>(data, at);
        } else {
            const size_t at = data.size() - 4 * (size_t)(count - shapeIndex + 1);
            if (at > data.size()) throw err("\"" + path + "\": corrupt offset dictionary");
            offset = leAt<uint32_t>(data, at);
        }
        if (offset + 4 > data.size()) throw err("\"" + path + "\": corrupt offset dictionary");
        header(offset);
    }
    Inflater z(data, offset + 4, path);
    const uint32_t flags = z.get<uint32_t>();
    if (version == 4) mesh.name = z.cstring();
    const uint64_t nv = z.get<uint64_t>(), nt = z.get<uint64_t>();
    if (nv > 0xFFFFFFFFull || nt > 0x7FFFFFFFull) throw err("\"" + path + "\": mesh too large for 32-bit indices");
    const bool dbl = (flags & kSerDouble) != 0;
    std::vector<float> buf;
    z.floats(buf, 3 * nv, dbl);
    mesh.p.resize(nv);
    for (size_t i = 0; i < nv; ++i) mesh.p[i] = V3(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]);
    mesh.n.clear();
    if (flags & kSerHasNormals) {
        z.floats(buf, 3 * nv, dbl);
        mesh.n.resize(nv);
        for (size_t i = 0; i < nv; ++i) mesh.n[i] = V3(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]);
    }
    mesh.uv.clear();
    if (flags & kSerHasTexcoords) z.floats(mesh.uv, 2 * nv, dbl);
    if (flags & kSerHasColors) z.floats(buf, 3 * nv, dbl);
    mesh.idx.resize(3 * nt);
    z.read(mesh.idx.data(), mesh.idx.size() * sizeof(uint32_t));
    for (uint32_t i : mesh.idx)
        if (i >= nv) throw err("\"" + path + "\": triangle index out of range");
}

// trimesh.cpp:608-681
static float unitAngle(const V3 &u, const V3 &v) {
    if (dot(u, v) < 0) return (float)M_PI - 2.0f * std::asin(0.5f * length(v + u));
    return 2.0f * std::asin(0.5f * length(v - u));
}

void computeNormals(Mesh &mesh, bool flipNormals) {
    if (mesh.faceNormals) {
        mesh.n.clear();
        if (flipNormals)
            for (size_t i = 0; i < mesh.idx.size(); i += 3) std::swap(mesh.idx[i], mesh.idx[i + 1]);
        return;
    }
    if (!mesh.n.empty()) {
        if (flipNormals) for (auto &n : mesh.n) n = -n;
        return;
    }
    mesh.n.assign(mesh.p.size(), V3(0.0f));
    for (size_t t = 0; t < mesh.idx.size(); t += 3) {
        V3 n(0.0f);
        for (int i = 0; i < 3; ++i) {
            const V3 &v0 = mesh.p[mesh.idx[t + i]];
            const V3 &v1 = mesh.p[mesh.idx[t + (i + 1) % 3]];
            const V3 &v2 = mesh.p[mesh.idx[t + (i + 2) % 3]];
            V3 sideA = v1 - v0, sideB = v2 - v0;
            if (i == 0) {
                n = cross(sideA, sideB);
                float len = length(n);
                if (len == 0) break;
                n /= len;
            }
            float angle = unitAngle(normalize(sideA), normalize(sideB));
            mesh.n[mesh.idx[t + i]] += n * angle;
        }
    }
    for (auto &n : mesh.n) {
        float len = length(n);
        if (flipNormals) len *= -1;
        if (len != 0) n /= len;
        else n = V3(1, 0, 0);
    }
}

void writePFM(const std::string &path, int w, int h, const std::vector<float> &rgb) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) throw err("cannot write " + path);
    fprintf(f, "PF\n%d %d\n-1\n", w, h);
    // PFM stores rows bottom-to-top (bitmap.cpp:347-398)
    for (int y = h - 1; y >= 0; --y) fwrite(&rgb[(size_t)y * w * 3], sizeof(float), (size_t)w * 3, f);
    fclose(f);
}

// ---------------------------------------------------------------------------
// Scene handler: XML -> Properties -> SceneBuilder (builder.cpp).  Mirrors
// SceneHandler (scenehandler.cpp:461-625 value tags, :700-780 objects): each
// element's values become its Properties, nested objects are created first
// (as the reference creates children before CreateInstance's caller adds
// them), named objects are kept in an id map for <ref>.
// ---------------------------------------------------------------------------
namespace {

struct Loader {
    SceneBuilder B;
    std::map<std::string, std::string> defines;
    std::map<std::string, int> bsdfIds;
    std::map<std::string, int> textureIds;
    std::map<std::string, int> groupIds;

    explicit Loader(Scene &s) : B(s) {}

    std::string subst(const std::string &v) {
        // $name substitution from -D / <default> (scenehandler.cpp:211)
        std::string o;
        for (size_t k = 0; k < v.size(); ++k) {
            if (v[k] == '$') {
                size_t e = k + 1;
                while (e < v.size() && (isalnum((unsigned char)v[e]) || v[e] == '_')) ++e;
                std::string key = v.substr(k + 1, e - k - 1);
                auto it = defines.find(key);
                if (it == defines.end()) throw err("Unresolved parameter \"$" + key + "\"");
                o += it->second;
                k = e - 1;
            } else {
                o += v[k];
            }
        }
        return o;
    }

    void substAll(XNode &n) {
        for (auto &a : n.attrs) a.second = subst(a.second);
    }

    Transform parseTransform(XNode &n) {
        Transform t;
        for (auto &cp : n.children) {
            XNode &c = *cp;
            substAll(c);
            const std::string &tag = c.tag;
            if (tag == "translate") {
                t = Transform::translate(V3(parseF(c.attr("x", "0"), c.line), parseF(c.attr("y", "0"), c.line), parseF(c.attr("z", "0"), c.line))) * t;
            } else if (tag == "rotate") {
                V3 ax(parseF(c.attr("x", "0"), c.line), parseF(c.attr("y", "0"), c.line), parseF(c.attr("z", "0"), c.line));
                t = Transform::rotate(ax, parseF(c.attr("angle"), c.line)) * t;
            } else if (tag == "scale") {
                bool hasXYZ = c.hasAttr("x") || c.hasAttr("y") || c.hasAttr("z");
                V3 s;
                if (hasXYZ && c.hasAttr("value")) throw err("<scale>: provided both xyz and value arguments!");
                if (hasXYZ) s = V3(parseF(c.attr("x", "1"), c.line), parseF(c.attr("y", "1"), c.line), parseF(c.attr("z", "1"), c.line));
                else if (c.hasAttr("value")) s = V3(parseF(c.attr("value"), c.line));
                else throw err("<scale>: provided neither xyz nor value arguments!");
                t = Transform::scale(s) * t;
            } else if (tag == "lookat" || tag == "lookAt") {
                auto o = tokenize(c.attr("origin"), ", "), tg = tokenize(c.attr("target"), ", "), up = tokenize(c.attr("up"), ", ");
                if (o.size() != 3) throw err("<lookat>: invalid 'origin' argument");
                if (tg.size() != 3) throw err("<lookat>: invalid 'target' argument");
                V3 O(parseF(o[0], c.line), parseF(o[1], c.line), parseF(o[2], c.line));
                V3 T(parseF(tg[0], c.line), parseF(tg[1], c.line), parseF(tg[2], c.line));
                V3 U(0.0f);
                if (up.size() == 3) U = V3(parseF(up[0], c.line), parseF(up[1], c.line), parseF(up[2], c.line));
                else if (!up.empty()) throw err("<lookat>: invalid 'up' argument");
                if (dot(U, U) == 0) { V3 unused; coordinateSystem(normalize(T - O), U, unused); }
                t = Transform::lookAt(O, T, U) * t;
            } else if (tag == "matrix") {
                auto tok = tokenize(c.attr("value"), ", ");
                if (tok.size() != 16) throw err("Invalid matrix specified");
                double m[4][4];
                for (int k = 0; k < 16; ++k) m[k / 4][k % 4] = parseF(tok[k], c.line);
                t = Transform::fromMatrix(m) * t;
            } else {
                throw err("line " + std::to_string(c.line) + ": unsupported transform element <" + tag + ">");
            }
        }
        return t;
    }

    V3 parseRGB(const std::string &v, int line) {
        auto tok = tokenize(v, ", ");
        if (tok.size() == 1 && tok[0].size() == 7 && tok[0][0] == '#') {
            int enc = (int)strtol(tok[0].c_str() + 1, nullptr, 16);
            return V3(((enc & 0xFF0000) >> 16) / 255.0f, ((enc & 0x00FF00) >> 8) / 255.0f, (enc & 0xFF) / 255.0f);
        }
        if (tok.size() == 1) return V3(parseF(tok[0], line));
        if (tok.size() == 3) return V3(parseF(tok[0], line), parseF(tok[1], line), parseF(tok[2], line));
        throw err("Invalid RGB value specified");
    }

    static float srgbToLinear(float v) {
        if (v <= 0.04045f) return v * (1.0f / 12.92f);
        return std::pow((v + 0.055f) * (1.0f / 1.055f), 2.4f);
    }

    // Parse value children of a plugin element into props; returns nested
    // plugin elements for the caller.
    void parseProps(XNode &n, Properties &props, std::vector<XNode *> &nested) {
        for (auto &cp : n.children) {
            XNode &c = *cp;
            substAll(c);
            if (!parseValue(c, props)) nested.push_back(&c);
        }
    }

    // one value element (<float>, <integer>, ... <transform>) into props;
    // false for any other element
    bool parseValue(XNode &c, Properties &props) {
        {
            const std::string name = c.attr("name");
            const std::string &tag = c.tag;
            if (tag == "float") props.floats[name] = parseF(c.attr("value"), c.line);
            else if (tag == "integer") {
                long long v = std::stoll(c.attr("value"));
                props.ints[name] = v;
            } else if (tag == "boolean") {
                std::string v = lower(c.attr("value"));
                if (v != "true" && v != "false") throw err("line " + std::to_string(c.line) + ": could not parse boolean \"" + v + "\"");
                props.bools[name] = v == "true";
            } else if (tag == "string") props.strings[name] = c.attr("value");
            else if (tag == "rgb") props.spectra[name] = parseRGB(c.attr("value"), c.line);
            else if (tag == "srgb") { V3 v = parseRGB(c.attr("value"), c.line); props.spectra[name] = V3(srgbToLinear(v.x), srgbToLinear(v.y), srgbToLinear(v.z)); }
            else if (tag == "spectrum") {
                if (c.hasAttr("filename")) throw err("<spectrum filename=...> is not supported in RGB mode by this loader");
                auto tok = tokenize(c.attr("value"), ", ");
                if (tok.size() == 1 && tok[0].find(':') == std::string::npos) {
                    // RGB mode: reflectance -> constant, illuminant -> D65 * v = v (spectrum.cpp:164)
                    props.spectra[name] = V3(parseF(tok[0], c.line));
                } else if (tok.size() == 3 && tok[0].find(':') == std::string::npos) {
                    props.spectra[name] = V3(parseF(tok[0], c.line), parseF(tok[1], c.line), parseF(tok[2], c.line));
                } else {
                    throw err("line " + std::to_string(c.line) + ": wavelength:value spectra are not supported by this loader");
                }
            } else if (tag == "point" || tag == "vector") {
                props.points[name] = V3(parseF(c.attr("x", "0"), c.line), parseF(c.attr("y", "0"), c.line), parseF(c.attr("z", "0"), c.line));
            } else if (tag == "transform") {
                props.transforms[name] = parseTransform(c);
            } else {
                return false;
            }
        }
        return true;
    }

    int parseTexture(XNode &n) {
        substAll(n);
        Properties props;
        std::vector<XNode *> nested;
        parseProps(n, props, nested);
        const int idx = B.texture(n.attr("type"), props, n.attr("id"), n.line);
        if (!n.attr("id").empty()) textureIds[n.attr("id")] = idx;
        return idx;
    }

    int parseBsdf(XNode &n) {
        substAll(n);
        Properties props;
        std::vector<XNode *> nested;
        parseProps(n, props, nested);
        const std::string type = lower(n.attr("type"));
        std::map<std::string, int> textures;
        std::vector<int> kids;
        for (XNode *c : nested) {
            substAll(*c);
            const std::string name = c->attr("name");
            if (c->tag == "texture") {
                textures[name] = parseTexture(*c);
            } else if (c->tag == "ref" && textureIds.count(c->attr("id"))) {
                textures[name] = textureIds[c->attr("id")];
            } else if (type == "twosided" && c->tag == "bsdf") {
                kids.push_back(parseBsdf(*c));
            } else if (type == "twosided" && c->tag == "ref") {
                const std::string id = c->attr("id");
                if (!bsdfIds.count(id)) throw err("Referenced object '" + id + "' not found!");
                kids.push_back(bsdfIds[id]);
            } else if (type == "twosided") {
                throw err("line " + std::to_string(c->line) + ": unsupported element <" + c->tag + "> inside twosided");
            } else if (c->tag != "bsdf" && c->tag != "ref") {
                throw err("line " + std::to_string(c->line) + ": unsupported element <" + c->tag + "> inside a BSDF");
            }
        }
        const int id = B.bsdf(type, props, textures, kids, n.attr("id"), n.line);
        if (!n.attr("id").empty()) bsdfIds[n.attr("id")] = id;
        return id;
    }

    int parseEmitter(XNode &n) {
        substAll(n);
        Properties props;
        std::vector<XNode *> nested;
        parseProps(n, props, nested);
        // a texture object among the children (SpotEmitter::addChild, spot.cpp:206-212)
        bool nestedTexture = false;
        for (XNode *c : nested)
            if (c->tag == "texture" || (c->tag == "ref" && textureIds.count(c->attr("id")))) nestedTexture = true;
        return B.emitter(n.attr("type"), props, n.line, nestedTexture);
    }

    void parseShape(XNode &n, int group) {
        substAll(n);
        std::string type = lower(n.attr("type"));
        if (type == "shapegroup") {
            if (group >= 0) throw err("Nested instancing is not permitted");
            const int g = B.group(n.attr("id"));
            for (auto &cp : n.children) {
                substAll(*cp);
                if (cp->tag != "shape") throw err("shapegroup may only contain shapes");
                parseShape(*cp, g);
            }
            groupIds[n.attr("id")] = g;
            return;
        }
        Properties props;
        std::vector<XNode *> nested;
        parseProps(n, props, nested);
        int bsdf = -1, emitter = -1, instRef = -1;
        for (XNode *c : nested) {
            substAll(*c);
            if (c->tag == "bsdf") bsdf = parseBsdf(*c);
            else if (c->tag == "emitter") {
                if (group >= 0) throw err("emitters inside shapegroups are not supported");
                if (lower(c->attr("type")) != "area")
                    throw err("line " + std::to_string(c->line) + ": a shape's emitter must be an 'area' emitter");
                emitter = parseEmitter(*c);
            } else if (c->tag == "ref") {
                std::string id = c->attr("id");
                if (bsdfIds.count(id)) bsdf = bsdfIds[id];
                else if (groupIds.count(id)) instRef = groupIds[id];
                else throw err("Referenced object '" + id + "' not found!");
            } else {
                throw err("line " + std::to_string(c->line) + ": unsupported element <" + c->tag + "> inside <shape>");
            }
        }
        if (type == "instance") {
            if (instRef < 0) throw err("A reference to a 'shapegroup' must be specified!");
            if (group >= 0) throw err("Nested instancing is not permitted");
            B.instance(instRef, props.getTransform("toWorld", Transform()));
            return;
        }
        B.shape(type, props, bsdf, emitter, group, n.line);
    }

    void parseScene(XNode &root) {
        for (auto &cp : root.children) {
            XNode &c = *cp;
            substAll(c);
            const std::string &tag = c.tag;
            if (tag == "default") {
                std::string name = c.attr("name");
                if (!defines.count(name)) defines[name] = c.attr("value");
            } else if (tag == "include") {
                std::string path = B.resolve(c.attr("filename"));
                std::string src = readFile(path);
                XParser p(src, path);
                p.skipMisc();
                auto sub = p.element();
                B.dirStack.push_back(dirName(path));
                parseScene(*sub);
                B.dirStack.pop_back();
            } else if (tag == "integrator") {
                Properties props;
                std::vector<XNode *> nested;
                parseProps(c, props, nested);
                // multichannel's nested integrators, in document order
                // (MultiChannelIntegrator::addChild, multichannel.cpp:219-231)
                // ... and adaptive's one (AdaptiveIntegrator::addChild, adaptive.cpp:94-104)
                const bool adaptive = lower(c.attr("type")) == "adaptive";
                for (XNode *k : nested) {
                    substAll(*k);
                    if (k->tag != "integrator" || (lower(c.attr("type")) != "multichannel" && !adaptive))
                        throw err("line " + std::to_string(k->line) + ": unsupported element <" + k->tag + "> inside this <integrator>");
                    Properties kp;
                    std::vector<XNode *> kn;
                    parseProps(*k, kp, kn);
                    if (adaptive) {
                        if (!kn.empty() && lower(k->attr("type")) == "path")
                            throw err("line " + std::to_string(k->line) + ": adaptive: a child integrator with nested objects is not supported");
                        B.adaptiveChild(k->attr("type"), kp, k->line);
                        continue;
                    }
                    if (!kn.empty() && lower(k->attr("type")) != "multichannel")
                        throw err("line " + std::to_string(k->line) + ": multichannel: a child integrator with nested objects is not supported");
                    B.integratorChild(k->attr("type"), kp, k->line);
                }
                B.integrator(c.attr("type"), props, c.line);
            } else if (tag == "sensor" || tag == "camera") {
                parseSensor(c);
            } else if (tag == "bsdf") {
                parseBsdf(c);
            } else if (tag == "texture") {
                parseTexture(c);
            } else if (tag == "shape") {
                parseShape(c, -1);
            } else if (tag == "emitter") {
                if (lower(c.attr("type")) == "area")
                    throw err("line " + std::to_string(c.line) + ": emitter \"area\" outside a shape is outside this build's scope");
                parseEmitter(c);
            } else if (tag == "ref") {
                // scene-level refs are ignored
            } else if (Properties p; parseValue(c, p)) {
                // the Scene's own Properties (Scene::Scene(props), scene.cpp:47-83)
                B.sceneProps(p, c.line);
            } else {
                throw err("line " + std::to_string(c.line) + ": unsupported element <" + tag + ">");
            }
        }
    }

    void parseSensor(XNode &c) {
        Properties props;
        std::vector<XNode *> nested;
        parseProps(c, props, nested);
        B.sensor(c.attr("type"), props, c.line);
        for (XNode *n : nested) {
            substAll(*n);
            if (n->tag == "film") {
                Properties fp;
                std::vector<XNode *> fn;
                parseProps(*n, fp, fn);
                B.film(n->attr("type"), fp);
                for (XNode *r : fn) {
                    substAll(*r);
                    if (r->tag != "rfilter") throw err("unsupported element <" + r->tag + "> inside <film>");
                    Properties rp;
                    std::vector<XNode *> rn;
                    parseProps(*r, rp, rn);
                    B.rfilter(r->attr("type"), rp);
                }
            } else if (n->tag == "sampler") {
                Properties sp;
                std::vector<XNode *> sn;
                parseProps(*n, sp, sn);
                B.sampler(n->attr("type"), sp);
            } else {
                throw err("unsupported element <" + n->tag + "> inside <sensor>");
            }
        }
    }
};
}  // namespace

bool readPFM(const std::string &path, int &w, int &h, std::vector<float> &rgb, std::string &err) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { err = "cannot open " + path; return false; }
    auto token = [&](std::string &out) {
        out.clear();
        int c;
        while ((c = fgetc(f)) != EOF && isspace(c)) {}
        while (c != EOF && !isspace(c)) { out.push_back((char)c); c = fgetc(f); }
        return !out.empty();
    };
    std::string magic, ws, hs, ss;
    bool ok = token(magic) && token(ws) && token(hs) && token(ss);
    if (!ok || (magic != "PF" && magic != "Pf")) { fclose(f); err = "invalid PFM header"; return false; }
    const bool color = magic == "PF";
    w = atoi(ws.c_str()); h = atoi(hs.c_str());
    const float scaleAndOrder = (float)strtod(ss.c_str(), nullptr);
    if (w <= 0 || h <= 0) { fclose(f); err = "invalid PFM size"; return false; }
    const size_t ch = color ? 3 : 1, n = (size_t)w * h * ch;
    std::vector<float> data(n);
    if (fread(data.data(), sizeof(float), n, f) != n) { fclose(f); err = "truncated PFM"; return false; }
    fclose(f);
    if (scaleAndOrder > 0) {   // big endian
        for (auto &v : data) {
            uint32_t u;
            memcpy(&u, &v, 4);
            u = __builtin_bswap32(u);
            memcpy(&v, &u, 4);
        }
    }
    const float scale = std::fabs(scaleAndOrder);
    if (scale != 1) for (auto &v : data) v *= scale;
    rgb.assign((size_t)w * h * 3, 0.0f);
    for (int y = 0; y < h; ++y)   // flipVertically(): PFM rows are bottom-up
        for (int x = 0; x < w; ++x)
            for (int k = 0; k < 3; ++k)
                rgb[((size_t)y * w + x) * 3 + k] = data[((size_t)(h - 1 - y) * w + x) * ch + (color ? k : 0)];
    return true;
}

int g_defaultKDThreads = 0;
int g_instancing = 0;

std::unique_ptr<Scene> loadScene(const std::string &path, const std::map<std::string, std::string> &defines,
                                 const mtsh_scene_overrides *ov, const Properties *sceneProps) {
    auto scene = SceneBuilder::newScene();
    Loader L(*scene);
    L.defines = defines;
    L.B.dirStack.push_back(dirName(path));
    std::string src = readFile(path);
    XParser p(src, path);
    p.skipMisc();
    auto root = p.element();
    if (root->tag != "scene") throw err("root element must be <scene>");
    L.parseScene(*root);
    if (sceneProps) L.B.sceneProps(*sceneProps);
    L.B.finish(ov);
    return scene;
}

}  // namespace mtsh
