// Known-answer driver for the Aws::Crt::Checksum surface: the cases come from the command line
// (tests/test_cpp_dropin.py reads them from tests/golden/reference_known_answers.json), so the
// reference's known answers are checked where its own test files are not at hand.
//   ./known_answers NAME ALG INPUT_HEX EXPECTED_HEX [NAME ALG INPUT_HEX EXPECTED_HEX ...]
// ALG: crc32 | crc32c | crc64nvme (EXPECTED_HEX is the value) or xxhash64 | xxhash3_64 | xxhash3_128
// (EXPECTED_HEX is the digest as written to the output buffer; one-shot and streaming, seed 0).
#include <aws/crt/Api.h>
#include <aws/crt/checksum/CRC.h>
#include <aws/crt/checksum/XXHash.h>
#include <aws/testing/aws_test_harness.h>
#include <aws_crt_amd/checksums_batch.h>

#include <cstdlib>
#include <string>
#include <vector>

using namespace Aws::Crt;

static std::vector<uint8_t> s_unhex(const std::string &h)
{
    std::vector<uint8_t> v;
    for (size_t i = 0; i + 1 < h.size(); i += 2)
        v.push_back((uint8_t)std::strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return v;
}

static int s_hash_case(struct aws_allocator *allocator, const std::string &alg, ByteCursor cur,
                       const std::vector<uint8_t> &want)
{
    ByteBuf out;
    aws_byte_buf_init(&out, allocator, want.size());
    bool ok = alg == "xxhash64"     ? Checksum::ComputeXXHash64(cur, out)
              : alg == "xxhash3_64" ? Checksum::ComputeXXHash3_64(cur, out)
                                    : Checksum::ComputeXXHash3_128(cur, out);
    ASSERT_TRUE(ok);
    ASSERT_BIN_ARRAYS_EQUALS(want.data(), want.size(), out.buffer, out.len);
    aws_byte_buf_reset(&out, false);
    auto h = alg == "xxhash64"     ? Checksum::XXHash::CreateXXHash64(0, allocator)
             : alg == "xxhash3_64" ? Checksum::XXHash::CreateXXHash3_64(0, allocator)
                                   : Checksum::XXHash::CreateXXHash3_128(0, allocator);
    ASSERT_TRUE(h.Update(cur));
    ASSERT_TRUE(h.Digest(out));
    ASSERT_BIN_ARRAYS_EQUALS(want.data(), want.size(), out.buffer, out.len);
    aws_byte_buf_clean_up(&out);
    return AWS_OP_SUCCESS;
}

static int s_case(struct aws_allocator *allocator, const std::string &alg, const std::string &input_hex,
                  const std::string &expected_hex)
{
    ApiHandle handle(allocator);
    std::vector<uint8_t> data = s_unhex(input_hex);
    ByteCursor cur = aws_byte_cursor_from_array(data.data(), data.size());
    if (alg == "crc32")
        ASSERT_UINT_EQUALS(std::strtoull(expected_hex.c_str(), nullptr, 16), Checksum::ComputeCRC32(cur));
    else if (alg == "crc32c")
        ASSERT_UINT_EQUALS(std::strtoull(expected_hex.c_str(), nullptr, 16), Checksum::ComputeCRC32C(cur));
    else if (alg == "crc64nvme")
        ASSERT_UINT_EQUALS(std::strtoull(expected_hex.c_str(), nullptr, 16), Checksum::ComputeCRC64NVME(cur));
    else if (alg == "xxhash64" || alg == "xxhash3_64" || alg == "xxhash3_128")
        return s_hash_case(allocator, alg, cur, s_unhex(expected_hex));
    else
        AWS_HARNESS_FAIL("unknown algorithm %s", alg.c_str());
    return AWS_OP_SUCCESS;
}

int main(int argc, char **argv)
{
    if (argc < 5 || (argc - 1) % 4 != 0)
    {
        std::fprintf(stderr, "usage: %s NAME ALG INPUT_HEX EXPECTED_HEX ...\n", argv[0]);
        return 2;
    }
    int failed = 0, ran = 0;
    for (int i = 1; i + 3 < argc; i += 4)
    {
        ++ran;
        int rc = s_case(aws_default_allocator(), argv[i + 1], argv[i + 2], argv[i + 3]);
        std::printf("[%s] %s\n", rc == AWS_OP_SUCCESS ? "PASS" : "FAIL", argv[i]);
        if (rc != AWS_OP_SUCCESS)
            ++failed;
    }
    std::printf("%d ran, %d failed\n", ran, failed);
    // where the single-buffer ABI ran (a forced-GPU run must have fallen back 0 times)
    std::printf("dispatch %d, gpu fallbacks %llu\n", aws_crt_amd_get_dispatch(), aws_crt_amd_fallback_count());
    return failed ? 1 : 0;
}
