// obj_parser.hpp — C++ restatement of the reference's Wavefront OBJ loader
// (raytracer/src/obj_parser/mod.rs:15-200), the front-end of its `teapot`
// demo. Same records and the same quirks:
//   * `v x y z` and `vn x y z` append to 1-based lists (index 0 is padding,
//     mod.rs:30-31); `g name` selects, and (re)creates, a named group;
//   * `f` with plain indices makes Triangles, with `a/b/c` or `a//c` fields
//     (decided by a '/' anywhere in the line, mod.rs:63) SmoothTriangles from the
//     first and the last field of each item; polygons are fan-triangulated
//     about their first vertex (mod.rs:102-136);
//   * any other non-empty line counts as ignored.
// Two deliberate differences:
//   * as_group() with named groups: the reference drains a HashMap
//     (mod.rs:138-148), so its child order is unspecified; here the children
//     are the non-empty groups in the order of their first `g` line.
//   * malformed numbers, missing fields and indices past the lists raise
//     RtError (RT_ERR_INVALID_ARGUMENT); the reference panics.
#pragma once
#include <cerrno>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "rt_world.hpp"

namespace rt {

class ObjParser {
 public:
  size_t ignored = 0;
  std::vector<Point> vertices{Point::origin()};
  std::vector<Vector> normals{Vector(0, 0, 0)};

  ObjParser() { groups_.push_back({"default", Group()}); }
  void parse(const std::string& contents) {  // mod.rs:38-42 (str::lines: '\n', a trailing '\r' dropped)
    size_t at = 0;
    while (at < contents.size()) {
      size_t nl = contents.find('\n', at);
      if (nl == std::string::npos) nl = contents.size();
      size_t end = nl;
      if (end > at && contents[end - 1] == '\r') --end;
      parse_line(contents.substr(at, end - at));
      at = nl + 1;
    }
  }
  void parse_line(const std::string& line) {  // mod.rs:44-100
    std::vector<std::string> items = split_ws(line);
    if (items.empty()) return;
    const std::string kind = items[0];
    items.erase(items.begin());
    if (kind == "v" || kind == "vn") {
      double n[3];
      if (items.size() < 3) bad(line, "needs three numbers");
      for (size_t i = 0; i < items.size(); ++i) {  // (every field is parsed, the first three are used)
        const double x = number(items[i], line);
        if (i < 3) n[i] = x;
      }
      if (kind == "v") vertices.push_back(Point(n[0], n[1], n[2]));
      else normals.push_back(Vector(n[0], n[1], n[2]));
    } else if (kind == "f") {
      if (items.size() < 2) bad(line, "a face needs at least two vertices");  // (1..len-1 underflows there)
      Group& g = selected();
      if (line.find('/') == std::string::npos) {
        std::vector<size_t> v;
        for (const std::string& it : items) v.push_back(index(it, vertices.size(), line));
        for (size_t i = 1; i + 1 < v.size(); ++i)
          g.add_child(Triangle(vertices[v[0]], vertices[v[i]], vertices[v[i + 1]]));
      } else {
        std::vector<size_t> v, n;
        for (const std::string& it : items) {  // split('/'): the first field and the last
          const size_t a = it.find('/'), b = it.rfind('/');
          v.push_back(index(it.substr(0, a), vertices.size(), line));
          n.push_back(index(b == std::string::npos ? it : it.substr(b + 1), normals.size(), line));
        }
        for (size_t i = 1; i + 1 < v.size(); ++i)
          g.add_child(SmoothTriangle(vertices[v[0]], vertices[v[i]], vertices[v[i + 1]], normals[n[0]], normals[n[i]],
                                     normals[n[i + 1]]));
      }
    } else if (kind == "g") {
      if (items.empty()) bad(line, "a group needs a name");
      selected_ = items[0];
      for (auto& ng : groups_)
        if (ng.first == selected_) {
          ng.second = Group();  // HashMap::insert replaces the group of that name
          return;
        }
      groups_.push_back({selected_, Group()});
    } else {
      ++ignored;
    }
  }
  // the group of that name ("default": the faces before any `g` line)
  const Group& group(const std::string& name) const {
    for (const auto& ng : groups_)
      if (ng.first == name) return ng.second;
    throw RtError(RT_ERR_INVALID_ARGUMENT, "ObjParser: no group named `" + name + "`");
  }
  std::vector<std::string> group_names() const {
    std::vector<std::string> v;
    for (const auto& ng : groups_) v.push_back(ng.first);
    return v;
  }
  // mod.rs:138-148: the default group alone, or a group of the non-empty groups
  // (in the order of their `g` lines). Like the reference's, it empties the parser's groups.
  Group as_group() {
    if (groups_.size() == 1) {
      Group g = std::move(groups_[0].second);
      groups_.clear();
      return g;
    }
    Group group;
    for (auto& ng : groups_)
      if (!ng.second.children.empty()) group.add_child(ng.second);
    groups_.clear();
    return group;
  }

 private:
  [[noreturn]] static void bad(const std::string& line, const std::string& why) {
    throw RtError(RT_ERR_INVALID_ARGUMENT, "ObjParser: " + why + " in `" + line + "`");
  }
  static std::vector<std::string> split_ws(const std::string& s) {  // split_ascii_whitespace
    std::vector<std::string> out;
    size_t i = 0;
    auto ws = [](char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f'; };
    while (i < s.size()) {
      while (i < s.size() && ws(s[i])) ++i;
      size_t j = i;
      while (j < s.size() && !ws(s[j])) ++j;
      if (j > i) out.push_back(s.substr(i, j - i));
      i = j;
    }
    return out;
  }
  static double number(const std::string& s, const std::string& line) {  // str::parse::<f64>
    if (s.empty() || s.find_first_of("xX") != std::string::npos) bad(line, "bad number `" + s + "`");
    char* end = nullptr;
    const double v = std::strtod(s.c_str(), &end);
    if (end != s.c_str() + s.size()) bad(line, "bad number `" + s + "`");
    return v;
  }
  static size_t index(const std::string& s, size_t size, const std::string& line) {  // str::parse::<usize>
    size_t i = !s.empty() && s[0] == '+' ? 1 : 0;
    if (i >= s.size() || s.size() - i > 18) bad(line, "bad index `" + s + "`");
    size_t v = 0;
    for (; i < s.size(); ++i) {
      if (s[i] < '0' || s[i] > '9') bad(line, "bad index `" + s + "`");
      v = v * 10 + (size_t)(s[i] - '0');
    }
    if (v >= size) bad(line, "index " + s + " is past the list");
    return v;
  }
  Group& selected() {
    for (auto& ng : groups_)
      if (ng.first == selected_) return ng.second;
    throw RtError(RT_ERR_INVALID_ARGUMENT, "ObjParser: the groups were taken by as_group()");
  }
  std::vector<std::pair<std::string, Group>> groups_;  // in the order of their `g` lines
  std::string selected_ = "default";
};

inline ObjParser parse_obj_string(const std::string& text) {
  ObjParser p;
  p.parse(text);
  return p;
}
inline ObjParser parse_obj_file(const std::string& path) {  // mod.rs:183-188
  std::ifstream f(path, std::ios::binary);
  if (!f) throw RtError(RT_ERR_INVALID_ARGUMENT, "ObjParser: cannot read `" + path + "`");
  std::stringstream ss;
  ss << f.rdbuf();
  return parse_obj_string(ss.str());
}

}  // namespace rt
