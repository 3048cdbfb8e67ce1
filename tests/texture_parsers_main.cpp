// texture_parsers_main.cpp -- a stand-alone program over the OBJ / MTL loader and ugrt_read_ppm, for a build of
// ugrt_host.cpp with -fsanitize=address,undefined (tests/test_texture.py compiles and runs it; nothing is loaded into
// Python).  Every argument is a file: a name that ends in .obj is loaded as a model and every list the loader exports is
// read from end to end, anything else is read as a PPM -- for its size, into a buffer of exactly 3 w h bytes and into one
// that is a byte short.  Return codes of the library are printed, not judged: the malformed files are meant to fail; the
// program exits 0 unless a sanitizer stops it.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ugrt.h"

static long long g_sum = 0; // (what is read is used, so that no read is optimised away)

static void model(const char *path)
{
	ugrt_scene *s = nullptr;
	if (ugrt_scene_create(&s))
		return;
	const int rc = ugrt_scene_load_model(s, path);
	int nv = 0, nf = 0, nm = 0, nt = 0, mtl = 0;
	ugrt_scene_counts(s, &nv, &nf, &nm);
	const float *uv = ugrt_scene_uvlist(s, &nt);
	const int *uf = ugrt_scene_uv_facelist(s), *fl = ugrt_scene_facelist(s), *mi = ugrt_scene_materiallist_index(s);
	const float *vl = ugrt_scene_vertexlist(s);
	ugrt_scene_reflectlist(s, &mtl);
	if (rc == UGRT_OK) {
		for (int i = 0; i < 2 * nt; i++)
			g_sum += uv[i] > 0.5f;
		for (int i = 0; i < 3 * nf; i++)
			g_sum += uf[i] + fl[i];
		for (int i = 0; i < nf; i++)
			g_sum += mi[i];
		for (int i = 0; i < 3 * nv; i++)
			g_sum += vl[i] > 0.0f;
	}
	for (int m = -1; m <= mtl; m++)
		g_sum += (long long)strlen(ugrt_scene_texture_name(s, m));
	g_sum += (long long)strlen(ugrt_scene_texture_dir(s));
	printf("%s: load_model %d, %d vertices, %d faces, %d vt, %d mtl materials\n", path, rc, nv, nf, nt, mtl);
	ugrt_scene_destroy(s);
}

static void ppm(const char *path)
{
	int w = 0, h = 0;
	const int rc0 = ugrt_read_ppm(path, &w, &h, nullptr, 0);
	int rc1 = -1, rc2 = -1;
	if (rc0 == UGRT_OK) {
		const size_t total = (size_t)3 * w * h;
		std::vector<unsigned char> exact(total), tight(total - 1);
		rc1 = ugrt_read_ppm(path, &w, &h, exact.data(), exact.size());
		rc2 = ugrt_read_ppm(path, &w, &h, tight.data(), tight.size());
		for (unsigned char b : exact)
			g_sum += b;
	}
	g_sum += ugrt_read_ppm(path, nullptr, &h, nullptr, 0) + ugrt_read_ppm(nullptr, &w, &h, nullptr, 0);
	printf("%s: read_ppm %d (%d x %d), full %d, a byte short %d\n", path, rc0, w, h, rc1, rc2);
}

int main(int argc, char **argv)
{
	for (int i = 1; i < argc; i++) {
		const std::string a(argv[i]);
		if (a.size() > 4 && a.compare(a.size() - 4, 4, ".obj") == 0)
			model(argv[i]);
		else
			ppm(argv[i]);
	}
	printf("done %lld\n", g_sum);
	return 0;
}
