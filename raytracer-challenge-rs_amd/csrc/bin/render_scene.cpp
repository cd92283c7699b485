// render_scene — the reference's scene-parser/src/bin/render_scene.rs on the
// MI355X path: `render_scene <scene-file> <output-file>` parses the YAML scene
// (csrc/host/scene_parser.hpp) and renders it with Camera::render through the
// C-ABI (GPU). An output path ending in .png gets a PNG, as the reference writes; any
// other path gets the P3 PPM (SceneParser::render_to). `--compress` after the output path
// makes the PNG the compressed one (rt_render_png_deflate).
#include <cstdio>
#include <cstring>
#include <exception>

#include "../host/scene_parser.hpp"

int main(int argc, char** argv) {
  const bool compress = argc == 4 && std::strcmp(argv[3], "--compress") == 0;
  if (argc != 3 && !compress) {
    std::printf("usage: render_scene <scene-file> <output-file> [--compress]\n");
    return 2;
  }
  try {
    rt::SceneParser parser;
    parser.load_file(argv[1]);
    for (const auto& m : parser.messages) std::printf("%s\n", m.c_str());
    parser.render_to(argv[2], 5, compress);
    std::printf("scene saved to %s\n", argv[2]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "Error: %s\n", e.what());
    return 1;
  }
  return 0;
}
